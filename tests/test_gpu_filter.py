"""GPU: vkv_filter_volume (3x3x3 binomial and median) byte for byte against the numpy restatements of
tests/test_filter_cpu.py (binomial3_np, median3_np).

k_filter3 works in tiles of 256 x 4 voxels (four waves, each 64 lanes of four x-adjacent voxels of one row) that march over 18 slices; a lane
loads the dword of its voxels (moved inwards and shifted where it would leave the row; widths below 4 gather bytes) and takes its outer
columns from the neighbouring lanes, the first and last lane of a wave from a byte load.  The extents below put the width at 1 .. 8, around
64 and 128 (a last lane with 1 .. 3 voxels) and at 255, 256, 257 (the wave's last lane on, and the next wave's first lane past, the row's
end); heights at 1 .. 5 and depths at 1 .. 3 and 17, 18, 19, so every tile dimension is met from one below, on and one above, and
257 x 5 x 19 spans two workgroups on every axis.  Every buffer is a tests/helpers.py guarded() allocation: an output is compared as a whole (an
unwritten byte shows as the pre-fill) and its guards must be intact, so nothing here relies on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_filter_cpu import CONTENTS, binomial3_np, contents, median3_np
from tests.test_gpu_mip import assert_same_bits, draw, make_volume, subpass
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu
KINDS = ((abi.FILTER_BINOMIAL3, binomial3_np, "binomial"), (abi.FILTER_MEDIAN3, median3_np, "median"))
SENTINEL = 0xA5


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


def run(ctx, vol, kind, box=None, src_offset=0, dst_offset=0, fill=0x00, what=""):
    """d_dst (pre-filled with SENTINEL) after vkv_filter_volume of `vol`, both buffers guarded; the guards must be intact"""
    d_src, h_src = T.guarded(vol, src_offset, fill, "cuda")
    d_dst, h_dst = T.guarded(np.full(vol.shape, SENTINEL, np.uint8), dst_offset, fill, "cuda")
    ctx.filter_volume(d_src.data_ptr(), d_dst.data_ptr(), ext_of(vol), box, kind, st())
    torch.cuda.synchronize()
    for name, h in (("d_src", h_src), ("d_dst", h_dst)):
        bad = h.check()
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    assert np.array_equal(d_src.cpu().numpy(), vol), "%s: the source changed" % what
    return d_dst.cpu().numpy()


def same(got, want, what):
    assert np.array_equal(got, want), "%s: %d bytes differ, first at (z, y, x) %s: got %s want %s" % (
        what, int((got != want).sum()), np.argwhere(got != want)[:4].tolist(), got[got != want][:4].tolist(), want[got != want][:4].tolist())


# ---- extents and contents ---------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1, 1), (1, 3, 2), (2, 1, 3), (3, 2, 1), (4, 4, 4), (5, 3, 19), (7, 5, 3), (8, 1, 1), (63, 4, 2), (64, 5, 17), (65, 3, 18),
           (67, 2, 3), (129, 5, 3), (255, 3, 2), (256, 4, 1), (257, 5, 19)]  # (width, height, depth)


@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_and_content_both_kinds(ctx, extent):
    w, h, d = extent
    for k, content in enumerate(CONTENTS):
        vol = contents(content, (d, h, w), seed=500 + k)
        for kind, ref, name in KINDS:
            what = "%s %s %s" % (name, content, extent)
            same(run(ctx, vol, kind, what=what), ref(vol), what)


# ---- alignment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(7, 3, 2), (261, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_pointer_alignment_with_both_guard_fills(ctx, extent):
    """odd widths: a row's tail and the next row's head share a dword.  The kernel's widest access is a dword, so the source and the
    output at +0 .. +3 each, and a few offsets up to +7; guard fills 0x00 and 0xFF: a result that consumed a guard byte
    differs under one of them"""
    w, h, d = extent
    vol = contents("random", (d, h, w), seed=77)
    offsets = [(s, t) for s in range(4) for t in range(4)] + [(5, 0), (7, 2), (0, 5), (3, 7)]
    for kind, ref, name in KINDS:
        want = ref(vol)
        for fill in (0x00, 0xFF):
            for s, t in offsets:
                what = "%s %s src +%d dst +%d fill %#x" % (name, extent, s, t, fill)
                same(run(ctx, vol, kind, src_offset=s, dst_offset=t, fill=fill, what=what), want, what)


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
BOX_VOLUME = (301, 9, 20)  # (width, height, depth)
BOXES = {
    "interior voxel": (100, 4, 10, 1, 1, 1), "corner 0": (0, 0, 0, 1, 1, 1), "corner 1": (300, 8, 19, 1, 1, 1),
    "face x0": (0, 4, 10, 1, 1, 1), "face x1": (300, 4, 10, 1, 1, 1), "face y0": (100, 0, 10, 1, 1, 1), "face y1": (100, 8, 10, 1, 1, 1),
    "face z0": (100, 4, 0, 1, 1, 1), "face z1": (100, 4, 19, 1, 1, 1),
    "across tiles, tail of 2": (3, 2, 1, 290, 6, 19),        # more than one tile on every axis; 290 = 256 + 8 lanes + 2 voxels
    "tail of 3 up to the last byte": (294, 7, 18, 7, 2, 2),  # the box ends with the volume: a dword stored at its tail would leave the payload
    "whole volume": (0, 0, 0, 301, 9, 20),
}


@pytest.fixture(scope="module")
def box_case():
    w, h, d = BOX_VOLUME
    vol = contents("random", (d, h, w), seed=91)
    return vol, {kind: ref(vol) for kind, ref, _ in KINDS}


@pytest.mark.parametrize("box", sorted(BOXES), ids=lambda b: b.replace(" ", "_").replace(",", ""))
def test_a_box_writes_exactly_its_voxels(ctx, box_case, box):
    vol, refs = box_case
    x0, y0, z0, w, h, d = BOXES[box]
    for kind, _, name in KINDS:
        want = np.full(vol.shape, SENTINEL, np.uint8)
        want[z0:z0 + d, y0:y0 + h, x0:x0 + w] = refs[kind][z0:z0 + d, y0:y0 + h, x0:x0 + w]
        for dst_offset in (0, 1):
            what = "%s box %s dst +%d" % (name, box, dst_offset)
            same(run(ctx, vol, kind, box=abi.Box(*BOXES[box]), dst_offset=dst_offset, fill=0x3C, what=what), want, what)


# ---- keeping a filtered copy current ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ref,name", KINDS, ids=[k[2] for k in KINDS])
def test_region_update_then_grown_box_equals_a_full_refilter(ctx, kind, ref, name):
    w, h, d = 70, 11, 19
    vol = contents("random", (d, h, w), seed=5)
    v = make_volume(ctx, vol, packed=False)
    copy = v.filter(kind)
    for origin, shape_dhw in (((5, 3, 2), (4, 2, 3)), ((0, 0, 0), (1, 1, 1)), ((66, 9, 15), (4, 2, 4)), ((0, 4, 17), (2, 7, 70))):
        x, y, z = origin
        bd, bh, bw = shape_dhw
        new = contents("random", shape_dhw, seed=x + 31 * y)
        vol[z:z + bd, y:y + bh, x:x + bw] = new
        v.update_region(origin, new, abi.SKIP_NONE)
        x0, y0, z0 = max(x - 1, 0), max(y - 1, 0), max(z - 1, 0)
        x1, y1, z1 = min(x + bw + 1, w), min(y + bh + 1, h), min(z + bd + 1, d)
        assert v.filter(kind, out=copy, box=((x0, y0, z0), (x1 - x0, y1 - y0, z1 - z0))) is copy
        torch.cuda.synchronize()
        assert np.array_equal(v.volume.cpu().numpy(), vol)
        same(copy.cpu().numpy(), ref(vol), "%s after the update at %s" % (name, origin))
    same(v.filter(kind).cpu().numpy(), copy.cpu().numpy(), "%s: full refilter" % name)
    two = v.filter(kind, passes=3)
    torch.cuda.synchronize()
    same(two.cpu().numpy(), ref(ref(ref(vol))), "%s: three passes" % name)


# ---- the result is an ordinary volume ---------------------------------------------------------------------------------------------------
def test_filtered_volume_renders_through_the_max_map_like_the_dense_mip(ctx):
    vol = contents("salt", (40, 44, 48), seed=0)
    vol[10:30, 12:30, 8:40] = contents("random", (20, 18, 32), seed=1)
    v = make_volume(ctx, vol)
    filtered = v.filter(abi.FILTER_MEDIAN3)
    torch.cuda.synchronize()
    same(filtered.cpu().numpy(), median3_np(vol), "median of the scene")
    v2 = make_volume(ctx, filtered)
    sp, p = subpass(v2)
    dense, skipped = draw(sp, p, 0.2, 0.9, skip=False), draw(sp, p, 0.2, 0.9, skip=True)
    assert_same_bits(skipped, dense, "MIP of the filtered volume")
    assert dense["intensity"].max() > 0.2 and skipped["counts"][:, 2].sum() > 0        # something was drawn, something was skipped


# ---- capture ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ref,name", KINDS, ids=[k[2] for k in KINDS])
def test_one_call_captured_into_a_graph_replays(ctx, kind, ref, name):
    vol = contents("random", (17, 9, 131), seed=13)
    d_src = torch.from_numpy(vol).cuda()
    d_dst = torch.full(vol.shape, SENTINEL, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # one direct call on the capture stream
        ctx.filter_volume(d_src.data_ptr(), d_dst.data_ptr(), ext_of(vol), None, kind, s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.filter_volume(d_src.data_ptr(), d_dst.data_ptr(), ext_of(vol), None, kind, s.cuda_stream)
    torch.cuda.synchronize()
    for seed in (13, 14):  # the source rewritten in place, the output fresh, then the graph replayed
        if seed != 13:
            vol = contents("random", vol.shape, seed=seed)
            d_src.copy_(torch.from_numpy(vol))
        d_dst.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        same(d_dst.cpu().numpy(), ref(vol), "%s replay, seed %d" % (name, seed))


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    n = w * h * d
    buf = torch.full((3 * n,), SENTINEL, dtype=torch.uint8, device="cuda")
    a, e = buf.data_ptr(), abi.Extent3D(w, h, d)
    bad = abi.VKV_E_INVALID_ARGUMENT
    for kind in (abi.FILTER_BINOMIAL3, abi.FILTER_MEDIAN3):
        assert ctx.filter_volume_rc(a, a + n - 1, e, None, kind, st()) == bad and "overlap" in ctx.last_error()
        assert ctx.filter_volume_rc(a + 1, a, e, None, kind, st()) == bad
        assert ctx.filter_volume_rc(a, a, e, None, kind, st()) == bad
        assert ctx.filter_volume_rc(a, a + n, e, abi.Box(0, 0, 0, 13, 1, 1), kind, st()) == bad and "box" in ctx.last_error()
        assert ctx.filter_volume_rc(a, a + n, e, abi.Box(11, 4, 3, 1, 2, 1), kind, st()) == bad
        assert ctx.filter_volume_rc(a, a + n, e, abi.Box(1, 1, 1, 1, 0, 1), kind, st()) == bad
        assert ctx.filter_volume_rc(None, a + n, e, None, kind, st()) == bad
        assert ctx.filter_volume_rc(a, None, e, None, kind, st()) == bad
        assert ctx.filter_volume_rc(a, a + n, abi.Extent3D(w, 0, d), None, kind, st()) == bad
    assert ctx.filter_volume_rc(a, a + n, e, None, 2, st()) == bad and "kind" in ctx.last_error()
    assert ctx.filter_volume_rc(a, a + n, e, None, -1, st()) == bad
    assert ctx.filter_volume_rc(a, a + n, abi.Extent3D(0x80000000, 1, 1), None, abi.FILTER_MEDIAN3, st()) == abi.VKV_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    # adjacent ranges do not overlap
    ctx.filter_volume(a, a + n, e, None, abi.FILTER_BINOMIAL3, st())
    torch.cuda.synchronize()
    assert bool((buf[:n] == SENTINEL).all()) and bool((buf[n:2 * n] == SENTINEL).all()) and bool((buf[2 * n:] == SENTINEL).all())
