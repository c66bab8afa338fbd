"""GPU: vkv_label_components and vkv_select_components bit for bit against the numpy statements of
tests/test_components_cpu.py (components_np, select_np): every label, every size, all three counts, every byte of the selected volume.

The kernels are one-dimensional over the box-linear voxel index: a wave's 64 consecutive voxels are one ENTRY (the tile, 64 x 1 x 1; it
wraps over rows where the box's width is no multiple of 64), linked by x-runs in the entry and merged with everything else through a
lock-free union-find; a workgroup holds four entries; a scan chunk holds 4096 entries = 262144 voxels.  The extents:
  1x1x1, 1x4x3, 3x1x4, 4x5x1, 2x2x2   the small and thin ones of the mesh tests: axes of length 1, fewer voxels than a wave;
  63, 64, 65, 127, 128, 129 x 3 x 2      one short of, at and one past one and two entries along x: a run ends with its entry, goes on over
                                        the seam, and (odd widths) entries start in the middle of a row and wrap;
  64x1x1, 64x2x1, 64x3x1, 64x1x2, 64x1x3, 64x2x3   at, one past and two past one tile in y and z (a tile is one row and one slice);
  255, 256, 257 x 2 x 2                  around one workgroup along x;
  5x7x67, 9x33x5                        narrow boxes: an entry spans many rows and several slices;
  64x65x64 (266240 voxels)              crosses a scan chunk: the second chunk's components take the first chunk's total;
  64x1024x1025 (67174400 voxels)        257 chunk sums, one more than a round of the scan of the chunk sums holds (closed-form references).
Sizes above one generation of workgroups, where merging workgroups are not all resident together: tests/test_gpu_components_scale.py.
Contents: below and above (nothing, one component), random densities 0.1, 0.31 (the cubic site-percolation threshold: large tortuous
components) and 0.6, the 3-D checkerboard (all singletons under 6, one component under 14 and 26), a ball, a serpentine (ONE
one-voxel-wide path through every row and slice: one component over every seam, with long find chains), two slabs joined by one voxel.
Every buffer is a tests/helpers.py guarded() allocation, pre-filled and compared as a whole (an unwritten element shows as the pre-fill, an
element past the written count must still hold it), all guards must be intact and the volume unchanged, so nothing here relies on, or can
cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_components_cpu import components_np, select_np
from tests.test_gpu_mesh import BOX_VOLUME, BOXES, FILL, ISO, block_extent, ext_of, sparse_volume, st
from tests.test_gpu_mesh_indexed import guard_damage, prefilled
from tests.test_gpu_mip import make_volume
from tests.test_mesh_cpu import ball, mesh_contents, mesh_np
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu

CONNECTIVITIES = (6, 14, 26)


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


# ---- contents ---------------------------------------------------------------------------------------------------------------------------
def serpentine(shape_dhw):
    """one path, one voxel wide: the even rows of the even slices in full, joined at alternating ends by one voxel of the odd rows; the odd
    slices hold one voxel, alternately at the path's end and at its start"""
    d, h, w = shape_dhw
    vol = np.full(shape_dhw, 17, np.uint8)
    vol[::2, ::2, :] = 255
    end = (0, w - 1)
    for k, y in enumerate(range(1, h, 2)):
        x = w - 1 if k % 2 == 0 else 0
        vol[::2, y, x] = 255
        end = (y, x)
    if (h - 1) % 2 == 0:        # the last row is a full one: the path ends at its far end
        end = (h - 1, (w - 1) if ((h - 1) // 2) % 2 == 0 else 0)
    for k, z in enumerate(range(1, d, 2)):
        y, x = end if k % 2 == 0 else (0, 0)
        vol[z, y, x] = 255
    return vol


def slabs(shape_dhw):
    d, h, w = shape_dhw
    vol = np.full(shape_dhw, 200, np.uint8)
    gap = max(w // 2 - 1, 0)
    vol[:, :, gap] = 17
    vol[d // 2, h // 2, gap] = 200
    return vol


def contents(kind, shape_dhw, seed=0):
    if kind in ("below", "above", "ball"):
        return mesh_contents(kind, shape_dhw, seed)
    if kind.startswith("random"):
        return np.where(np.random.default_rng(seed).random(shape_dhw) < float(kind.split()[1]), 200, 17).astype(np.uint8)
    if kind == "checkerboard":
        z, y, x = np.indices(shape_dhw)
        return np.where((x + y + z) % 2 == 0, 255, 0).astype(np.uint8)
    return {"serpentine": serpentine, "slabs": slabs}[kind](shape_dhw)


CONTENTS = ("below", "above", "random 0.1", "random 0.31", "random 0.6", "checkerboard", "ball", "serpentine", "slabs")


def test_the_contents_are_what_the_docstring_says():
    shape = (5, 7, 9)
    for c in CONNECTIVITIES:
        assert components_np(contents("serpentine", shape), ISO, c)[2][0] == 1
        assert components_np(contents("slabs", shape), ISO, c)[2][0] == 1
        assert components_np(contents("above", shape), ISO, c)[2].tolist() == [1, 1, 315]
        assert components_np(contents("below", shape), ISO, c)[2].tolist() == [0, 0, 0]
    s = contents("serpentine", shape)
    inside = s >= 128
    padded = np.pad(inside, 1).astype(np.int64)
    degree = sum(np.roll(padded, o, a) for a in range(3) for o in (1, -1))[1:-1, 1:-1, 1:-1]        # inside 6-neighbours
    assert int(((degree == 1) & inside).sum()) == 2 and int(((degree > 2) & inside).sum()) == 0        # a path: two ends, no branch
    cut = contents("slabs", shape)
    cut[2, 3, 3] = 17
    assert components_np(cut, ISO, 6)[2][0] == 2
    assert components_np(contents("checkerboard", shape), ISO, 6)[2][0] == 158 and components_np(contents("checkerboard", shape), ISO, 14)[2][0] == 1


# ---- one call ---------------------------------------------------------------------------------------------------------------------------
def run(ctx, vol, iso, connectivity, cap, box=None, block=0, vol_offset=0, vol_fill=0x00, null_sizes=False, map_extent=None, max_map=None, what=""):
    """(labels: the whole buffer, the box's shape, uint32; sizes: the whole buffer [max(cap, 1)] uint32; counts [3] uint64) of ONE
    vkv_label_components call on guarded buffers, every output pre-filled with FILL; with `block` through the max map of that block size, with
    `map_extent` (w, h, d) through the map of that extent (built here, or the bytes `max_map`)"""
    abox = None if box is None else abi.Box(*box)
    shape = vol.shape if box is None else (box[5], box[4], box[3])
    d_vol, h_vol = T.guarded(vol, vol_offset, vol_fill, "cuda")
    nbytes = lib.components_scratch_bytes(ext_of(vol), abox)
    assert nbytes >= 40 and nbytes % 8 == 0 and nbytes <= int(np.prod(shape)) + 64, (what, nbytes)
    d_scratch, h_scratch = T.guarded((nbytes // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_counts, h_counts = T.guarded((3,), 0, FILL, "cuda", dtype=np.int64)
    d_labels, h_labels = T.guarded(shape, 0, FILL, "cuda", dtype=np.int32)
    d_sizes, h_sizes = T.guarded((max(cap, 1),), 0, FILL, "cuda", dtype=np.int32)
    handles = [("d_volume", h_vol), ("d_scratch", h_scratch), ("d_counts", h_counts), ("d_labels", h_labels), ("d_sizes", h_sizes)]
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
    ctx.label_components(d_vol.data_ptr(), ext_of(vol), abox, iso, connectivity, None if d_map is None else d_map.data_ptr(), me, d_scratch.data_ptr(),
                         d_labels.data_ptr(), None if null_sizes else d_sizes.data_ptr(), cap, d_counts.data_ptr(), st())
    torch.cuda.synchronize()
    for name, h in handles:
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    assert np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    return d_labels.cpu().numpy().view(np.uint32), d_sizes.cpu().numpy().view(np.uint32), d_counts.cpu().numpy().view(np.uint64)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d elements differ, first at %s: got %s want %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(),
                                                                                 want[bad][:4].tolist())


def check(ctx, vol, iso, connectivity, want=None, cap=None, box=None, what="", **kw):
    """one call against the oracle: the labels, the exact prefix of the sizes and the pre-fill behind it, the three counts"""
    wl, ws, wc = components_np(vol, iso, connectivity, box) if want is None else want
    k = int(wc[0])
    cap = k + 5 if cap is None else cap
    labels, sizes, counts = run(ctx, vol, iso, connectivity, cap, box=box, what=what, **kw)
    written = min(k, cap)
    assert counts.tolist() == [k, written, int(wc[2])], "%s: counts %s, expected %s" % (what, counts.tolist(), [k, written, int(wc[2])])
    same(labels, wl, what + ": labels")
    es = prefilled(sizes.shape, np.uint32)
    es[:written] = ws[:written]
    same(sizes, es, what + ": sizes")
    return labels, sizes, counts


# ---- extents and contents ---------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1, 1), (1, 4, 3), (3, 1, 4), (4, 5, 1), (2, 2, 2),
           (63, 3, 2), (64, 3, 2), (65, 3, 2), (127, 3, 2), (128, 3, 2), (129, 3, 2),
           (64, 1, 1), (64, 2, 1), (64, 3, 1), (64, 1, 2), (64, 1, 3), (64, 2, 3),
           (255, 2, 2), (256, 2, 2), (257, 2, 2), (5, 7, 67), (9, 33, 5)]  # (width, height, depth)


@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_content_and_connectivity(ctx, extent):
    w, h, d = extent
    for k, content in enumerate(CONTENTS):
        vol = contents(content, (d, h, w), seed=900 + k)
        for c in CONNECTIVITIES:
            want = components_np(vol, ISO, c)
            what = "%s %s, %d" % (content, extent, c)
            if content == "below":
                assert want[2].tolist() == [0, 0, 0], what
            elif content in ("above", "serpentine"):
                assert want[2][0] == 1, what
            check(ctx, vol, ISO, c, want, what=what)


@pytest.fixture(scope="module")
def chunk_extent():
    return 64, 65, 64        # 266240 voxels = 4160 entries: one scan chunk and 64 entries of the next


@pytest.mark.parametrize("content", ["above", "random 0.1", "random 0.31", "checkerboard", "serpentine"])
def test_more_entries_than_one_scan_chunk(ctx, chunk_extent, content):
    w, h, d = chunk_extent
    vol = contents(content, (d, h, w), seed=41)
    for c in (CONNECTIVITIES if content == "random 0.31" else (6, 26)):
        want = components_np(vol, ISO, c)
        if content.startswith("random") and c == 6:
            assert want[0].reshape(-1)[262144:].max() > want[0].reshape(-1)[:262144].max() > 0        # components begin in both chunks
        check(ctx, vol, ISO, c, want, what="%s %s, %d" % (content, chunk_extent, c))


# ---- more chunk sums than one round of the scan -------------------------------------------------------------------------------------------
ROUNDS_EXTENT = (64, 1024, 1025)        # 67 174 400 voxels = 1 049 600 entries of 64 = 257 chunks of 4096: one more than a round of the scan holds


@pytest.fixture(scope="module")
def lattice():
    """inside exactly where x, y and z are all even: every component is one voxel under 6, 14 and 26, so K = 32 x 512 x 513, the label of an
    inside voxel is its running count in memory order and every size is 1 (closed forms: components_np does not run at this size)"""
    w, h, d = ROUNDS_EXTENT
    vol = np.zeros((d, h, w), np.uint8)
    vol[::2, ::2, ::2] = 255
    inside = vol.reshape(-1) != 0
    k = 32 * 512 * 513
    labels = np.where(inside, np.cumsum(inside, dtype=np.uint32), np.uint32(0)).reshape(vol.shape)
    assert int(labels.max()) == k == 8404992 and labels[d - 1, h - 2, w - 2] == k
    return vol, (labels, np.ones(k, np.uint32), np.array([k, k, k], np.uint64))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_more_chunk_sums_than_one_round_of_the_scan_lattice(ctx, lattice, connectivity):
    """257 chunk sums: k_cc_scan_total carries a total into a second round, and the last chunk's components are ranked behind 8 388 608 others;
    with capacity K - 1 the exact prefix of the sizes is written and nothing behind it"""
    vol, want = lattice
    k = int(want[2][0])
    check(ctx, vol, ISO, connectivity, want, cap=k, what="lattice %s, %d, capacity K" % (ROUNDS_EXTENT, connectivity))
    check(ctx, vol, ISO, connectivity, want, cap=k - 1, what="lattice %s, %d, capacity K - 1" % (ROUNDS_EXTENT, connectivity))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_more_chunk_sums_than_one_round_of_the_scan_sparse_rows(ctx, connectivity):
    """five full rows far apart, the last one the last entry of the 257th chunk: five components of 64 voxels, and the last one's label, 5,
    is the total that the scan carried over 256 chunk sums plus one"""
    w, h, d = ROUNDS_EXTENT
    vol = np.zeros((d, h, w), np.uint8)
    labels = np.zeros((d, h, w), np.uint32)
    rows = ((0, 0), (3, 1000), (512, 513), (1023, 0), (1024, 1023))
    for k, (z, y) in enumerate(rows):
        vol[z, y, :] = 255
        labels[z, y, :] = k + 1
    assert (rows[-1][0] * h + rows[-1][1]) // 4096 == 256 and (rows[-2][0] * h + rows[-2][1]) // 4096 < 256
    want = (labels, np.full(5, 64, np.uint32), np.array([5, 5, 320], np.uint64))
    check(ctx, vol, ISO, connectivity, want, what="sparse rows %s, %d" % (ROUNDS_EXTENT, connectivity))
    check(ctx, vol, ISO, connectivity, want, cap=4, what="sparse rows %s, %d, capacity 4" % (ROUNDS_EXTENT, connectivity))


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
MORE_BOXES = {"far corner, wide": (40, 2, 3, 261, 7, 17), "two entries and one voxel": (44, 1, 1, 129, 3, 3), "height 1 inside": (7, 4, 2, 9, 1, 5),
              "one voxel": (300, 8, 19, 1, 1, 1)}


@pytest.fixture(scope="module")
def box_volume():
    w, h, d = BOX_VOLUME
    return contents("random 0.45", (d, h, w), seed=91)


@pytest.mark.parametrize("box", sorted(BOXES) + sorted(MORE_BOXES), ids=lambda b: b.replace(" ", "_").replace(",", ""))
def test_a_box_is_labelled_as_the_cropped_array(ctx, box_volume, box):
    b = BOXES.get(box) or MORE_BOXES[box]
    x0, y0, z0, w, h, d = b
    crop = np.ascontiguousarray(box_volume[z0:z0 + d, y0:y0 + h, x0:x0 + w])
    for c in CONNECTIVITIES:
        want = components_np(crop, ISO, c)        # the faces cut the whole volume's components: only the box's voxels connect
        labels, _, _ = check(ctx, box_volume, ISO, c, want, box=b, what="box %s, %d" % (box, c))
        assert labels.shape == (d, h, w)
        check(ctx, box_volume, ISO, c, want, box=b, block=4, what="box %s, %d, max map" % (box, c))
    assert components_np(box_volume, ISO, 6, (40, 2, 3, 261, 7, 17))[2][0] != components_np(box_volume, ISO, 6)[2][0]


# ---- alignment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(7, 3, 3), (131, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_volume_alignment_with_both_guard_fills(ctx, extent):
    """a result that consumed a guard byte as a voxel differs under one of the two fills"""
    w, h, d = extent
    vol = contents("random 0.4", (d, h, w), seed=77)
    for c in (6, 26):
        want = components_np(vol, ISO, c)
        for fill in (0x00, 0xFF):
            for offset in (0, 1, 2, 3):
                check(ctx, vol, ISO, c, want, vol_offset=offset, vol_fill=fill, what="%s, %d, volume +%d fill %#x" % (extent, c, offset, fill))


# ---- max map ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [2, 4])
def test_max_map_gives_the_dense_bytes(ctx, block):
    vol = sparse_volume()
    for c in CONNECTIVITIES:
        want = components_np(vol, ISO, c)
        assert want[2][0] >= 3
        dense = check(ctx, vol, ISO, c, want, what="dense, %d" % c)
        sparse = check(ctx, vol, ISO, c, want, block=block, what="max map, block %d, %d" % (block, c))
        for a, b in zip(dense, sparse):
            assert np.array_equal(a, b)
        check(ctx, vol, ISO, c, want, block=block, cap=int(want[2][0]) // 2, what="max map, block %d, %d, short capacity" % (block, c))
    check(ctx, vol, 0.05, 6, block=block, what="max map, block %d, iso 0.05: nothing skipped" % block)
    empty = components_np(vol, 1.5, 26)
    assert empty[2].tolist() == [0, 0, 0]
    check(ctx, vol, 1.5, 26, empty, block=block, what="max map, block %d, nothing inside" % block)


def test_iso_on_a_voxel_value_and_the_extreme_isos(ctx):
    vol = np.random.default_rng(6).integers(120, 137, size=(5, 6, 70), dtype=np.uint8)
    iso = float(np.float32(128) * np.float32(1.0 / 255.0))
    for c in CONNECTIVITIES:
        check(ctx, vol, iso, c, what="iso = 128 / 255, %d" % c)
        check(ctx, vol, iso, c, block=2, what="iso = 128 / 255, %d, max map" % c)
    for iso in (0.0, -3.0, 1.0, 1.5):
        check(ctx, vol, iso, 6, what="iso %g" % iso)
    full = np.full((2, 3, 65), 255, np.uint8)
    check(ctx, full, 1.0, 14, what="iso 1 on bytes of 255")


# ---- capacities -------------------------------------------------------------------------------------------------------------------------
def test_capacities_give_exact_prefixes_and_the_exact_total(ctx):
    vol = contents("random 0.2", (18, 6, 70), seed=3)
    for c in CONNECTIVITIES:
        want = components_np(vol, ISO, c)
        k = int(want[2][0])
        assert k > 20
        for cap in (0, 1, k - 1, k, k + 5):
            labels, sizes, counts = check(ctx, vol, ISO, c, want, cap=cap, what="capacity %d of %d, %d" % (cap, k, c))
            assert counts[0] == k
        labels, sizes, counts = run(ctx, vol, ISO, c, 0, null_sizes=True, what="counting call")
        assert counts.tolist() == [k, 0, int(want[2][2])] and (sizes.view(np.uint8) == FILL).all()
        same(labels, want[0], "counting call: labels")


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_on_the_same_buffers_give_identical_bytes(ctx):
    vol = contents("random 0.31", (19, 5, 258), seed=21)
    d_vol = torch.from_numpy(vol).cuda()
    n = lib.components_scratch_bytes(ext_of(vol))
    d_scratch = torch.full((n // 8,), -1, dtype=torch.int64, device="cuda")
    for c in CONNECTIVITIES:
        wl, ws, wc = components_np(vol, ISO, c)
        k = int(wc[0])
        d_labels = torch.full(vol.shape, -1, dtype=torch.int32, device="cuda")
        d_sizes = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        d_counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        results = []
        for _ in range(2):        # the second run starts from the first run's labels, sizes and scratch
            ctx.label_components(d_vol.data_ptr(), ext_of(vol), None, ISO, c, None, None, d_scratch.data_ptr(), d_labels.data_ptr(), d_sizes.data_ptr(), k,
                                 d_counts.data_ptr(), st())
            torch.cuda.synchronize()
            results.append((d_labels.cpu().numpy().view(np.uint32), d_sizes.cpu().numpy().view(np.uint32), d_counts.cpu().numpy().view(np.uint64)))
        for a, b in zip(*results):
            assert np.array_equal(a, b)
        same(results[1][0], wl, "second run: labels")
        same(results[1][1], ws, "second run: sizes")
        assert results[1][2].tolist() == wc.tolist()


def test_one_call_captured_into_a_graph_replays(ctx):
    shape = (17, 9, 131)
    vol = contents("random 0.31", shape, seed=13)
    cap = 17 * 9 * 131
    d_vol = torch.from_numpy(vol).cuda()
    d_scratch = torch.empty((lib.components_scratch_bytes(ext_of(vol)) // 8,), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros((3,), dtype=torch.int64, device="cuda")
    d_labels = torch.empty(shape, dtype=torch.int32, device="cuda")
    d_sizes = torch.empty((cap,), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def call():
        ctx.label_components(d_vol.data_ptr(), ext_of(vol), None, ISO, 26, None, None, d_scratch.data_ptr(), d_labels.data_ptr(), d_sizes.data_ptr(), cap,
                             d_counts.data_ptr(), s.cuda_stream)

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
            vol = contents("random 0.31", shape, seed=seed)
            d_vol.copy_(torch.from_numpy(vol))
        for t in (d_labels, d_sizes):
            t.view(torch.uint8).fill_(FILL)
        d_counts.fill_(-1)
        d_scratch.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        wl, ws, wc = components_np(vol, ISO, 26)
        k = int(wc[0])
        assert d_counts.cpu().tolist() == [k, k, int(wc[2])] and 0 < k <= cap
        same(d_labels.cpu().numpy().view(np.uint32), wl, "replay, seed %d: labels" % seed)
        same(d_sizes[:k].cpu().numpy().view(np.uint32), ws, "replay, seed %d: sizes" % seed)
        assert bool((d_sizes[k:].view(torch.uint8) == FILL).all())


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")        # [scratch 2048 | counts 32 | sizes 2016 | labels 2048 | a volume 2048]
    a = out.data_ptr()
    assert a % 8 == 0 and lib.components_scratch_bytes(e) <= 2048
    scratch, counts, sizes, labels, dst, v = a, a + 2048, a + 2080, a + 4096, a + 6144, vol.data_ptr()
    me, none = abi.Extent3D(3, 2, 1), None
    bad, unsupported, inf, nan = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED, float("inf"), float("nan")
    rc = lambda *args: ctx.label_components_rc(*args, st())  # noqa: E731
    tail = (scratch, labels, sizes, 10, counts)
    assert rc(None, e, None, 0.5, 6, None, none, *tail) == bad
    assert rc(v, e, None, 0.5, 6, None, none, None, labels, sizes, 10, counts) == bad
    assert rc(v, e, None, 0.5, 6, None, none, scratch, None, sizes, 10, counts) == bad
    assert rc(v, e, None, 0.5, 6, None, none, scratch, labels, sizes, 10, None) == bad
    assert rc(v, e, None, 0.5, 6, None, none, scratch, labels, None, 10, counts) == bad and "d_sizes" in ctx.last_error()
    assert rc(v, e, None, 0.5, 6, None, none, scratch, labels, sizes, 1 << 32, counts) == bad and "32-bit" in ctx.last_error()
    assert rc(v, abi.Extent3D(w, 0, d), None, 0.5, 6, None, none, *tail) == bad
    for iso in (inf, -inf, nan):
        assert rc(v, e, None, iso, 6, None, none, *tail) == bad and "iso" in ctx.last_error()
    for c in (0, 4, 8, 18, 27, -6):
        assert rc(v, e, None, 0.5, c, None, none, *tail) == bad and "connectivity" in ctx.last_error()
    assert rc(v, e, abi.Box(0, 0, 0, 13, 2, 2), 0.5, 6, None, none, *tail) == bad and "box" in ctx.last_error()
    assert rc(v, e, abi.Box(11, 4, 3, 1, 2, 1), 0.5, 6, None, none, *tail) == bad
    assert rc(v, e, abi.Box(1, 1, 1, 2, 0, 2), 0.5, 6, None, none, *tail) == bad
    assert rc(v, e, None, 0.5, 6, v, none, *tail) == bad and "map_extent" in ctx.last_error()
    assert rc(v, e, None, 0.5, 6, v, abi.Extent3D(13, 2, 1), *tail) == bad
    assert rc(v, e, None, 0.5, 6, None, none, scratch + 4, labels, sizes, 10, counts) == bad and "aligned" in ctx.last_error()
    assert rc(v, e, None, 0.5, 6, None, none, scratch, labels + 2, sizes, 10, counts) == bad
    assert rc(v, e, None, 0.5, 6, None, none, scratch, labels, sizes + 1, 10, counts) == bad
    assert rc(v, e, None, 0.5, 6, None, none, scratch, labels, sizes, 10, counts + 4) == bad
    assert rc(v, abi.Extent3D(0x10000, 0x10000, 2), None, 0.5, 6, None, none, *tail) == unsupported        # 2^33 voxels
    assert rc(v, abi.Extent3D(0x10000, 0x10000, 1), None, 0.5, 6, None, none, *tail) == unsupported        # 2^32: one too many
    # vkv_select_components
    sel = lambda *args: ctx.select_components_rc(*args, st())  # noqa: E731
    assert sel(None, dst, e, None, labels, sizes, counts, 0, 10, 0) == bad
    assert sel(v, None, e, None, labels, sizes, counts, 0, 10, 0) == bad
    assert sel(v, dst, e, None, None, sizes, counts, 0, 10, 0) == bad
    assert sel(v, dst, e, None, labels, sizes, None, 0, 10, 0) == bad
    assert sel(v, dst, abi.Extent3D(0, h, d), None, labels, sizes, counts, 0, 10, 0) == bad
    assert sel(v, dst, e, abi.Box(0, 0, 0, 13, 2, 2), labels, sizes, counts, 0, 10, 0) == bad and "box" in ctx.last_error()
    assert sel(v, dst, e, abi.Box(1, 1, 1, 2, 0, 2), labels, sizes, counts, 0, 10, 0) == bad
    assert sel(v, dst, e, None, labels, sizes, counts, 0, 10, 256) == bad and "fill" in ctx.last_error()
    assert sel(v, dst, e, None, labels, sizes, counts, 11, 10, 0) == bad and "min_voxels" in ctx.last_error()
    assert sel(v, dst, e, None, labels + 2, sizes, counts, 0, 10, 0) == bad and "aligned" in ctx.last_error()
    assert sel(v, dst, e, None, labels, sizes + 1, counts, 0, 10, 0) == bad
    assert sel(v, dst, e, None, labels, sizes, counts + 4, 0, 10, 0) == bad
    for shift in (1, 100, w * h * d - 1):        # the two volumes overlap without being equal
        assert sel(dst, dst + shift, e, None, labels, sizes, counts, 0, 10, 0) == bad and "overlap" in ctx.last_error()
        assert sel(dst + shift, dst, e, None, labels, sizes, counts, 0, 10, 0) == bad
    assert sel(v, dst, abi.Extent3D(0x10000, 0x10000, 2), None, labels, sizes, counts, 0, 10, 0) == unsupported
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # and the accepted calls next to them, with a valid max map argument that is not used: one component of 240 voxels, removed in place
    assert rc(v, e, None, 0.5, 6, None, me, *tail) == abi.VKV_OK
    assert sel(v, v, e, None, labels, sizes, counts, 241, 1000, 7) == abi.VKV_OK
    torch.cuda.synchronize()
    assert out[2048:2072].view(torch.int64).tolist() == [1, 1, 240] and out[2080:2084].view(torch.int32).tolist() == [240]
    assert bool((out[2084:4096] == FILL).all()) and bool((out[4096:4096 + 960].view(torch.int32) == 1).all()) and bool((out[4096 + 960:] == FILL).all())
    assert bool((vol == 7).all())


# ---- vkv_select_components --------------------------------------------------------------------------------------------------------------
def select(ctx, vol, labels, sizes, counts, lo, hi, fill, box=None, in_place=False, null_sizes=False, what=""):
    """the whole destination volume of ONE vkv_select_components call on guarded buffers (the destination pre-filled with FILL unless in place)"""
    abox = None if box is None else abi.Box(*box)
    d_src, h_src = T.guarded(vol, 1, FILL, "cuda")
    d_dst, h_dst = (d_src, h_src) if in_place else T.guarded(vol.shape, 3, FILL, "cuda")
    d_labels, h_labels = T.guarded(labels.view(np.int32), 0, FILL, "cuda")
    d_sizes, h_sizes = T.guarded(np.ascontiguousarray(sizes if len(sizes) else np.zeros(1, np.uint32)).view(np.int32), 0, FILL, "cuda")
    d_counts, h_counts = T.guarded(counts.view(np.int64), 0, FILL, "cuda")
    ctx.select_components(d_src.data_ptr(), d_dst.data_ptr(), ext_of(vol), abox, d_labels.data_ptr(), None if null_sizes else d_sizes.data_ptr(),
                          d_counts.data_ptr(), lo, hi, fill, st())
    torch.cuda.synchronize()
    for name, h in (("d_src", h_src), ("d_dst", h_dst), ("d_labels", h_labels), ("d_sizes", h_sizes), ("d_counts", h_counts)):
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed" % (what, name, bad[:8])
    if not in_place:
        assert np.array_equal(d_src.cpu().numpy(), vol), "%s: the source changed" % what
    assert np.array_equal(d_labels.cpu().numpy().view(np.uint32), labels) and np.array_equal(d_counts.cpu().numpy().view(np.uint64), counts)
    return d_dst.cpu().numpy()


EVERYTHING = 2 ** 64 - 1


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_select_against_the_statement(ctx, connectivity):
    vol = contents("random 0.2", (9, 7, 131), seed=5)
    vol[vol > 128] = np.random.default_rng(1).integers(128, 256, size=int((vol > 128).sum()), dtype=np.uint8)        # not one value: src is copied
    labels, sizes, counts = check(ctx, vol, ISO, connectivity, what="labels for select")
    k = int(counts[0])
    sizes = sizes[:k]
    assert k > 20 and sizes.max() > 4 and (sizes == 1).sum() > 5
    fresh = np.full(vol.shape, FILL, np.uint8)
    for lo, hi, fill in ((3, EVERYTHING, 0), (0, 2, 0), (2, 4, 9), (0, EVERYTHING, 1), (int(sizes.max()), EVERYTHING, 0), (int(sizes.max()) + 1, EVERYTHING, 255)):
        want = select_np(vol, labels, sizes, k, lo, hi, fill)
        what = "select [%d, %d] fill %d, %d" % (lo, hi, fill, connectivity)
        same(select(ctx, vol, labels, sizes, counts, lo, hi, fill, what=what), want, what)
        same(select(ctx, vol, labels, sizes, counts, lo, hi, fill, in_place=True, what=what + ", in place"), want, what + ", in place")
    assert (select_np(vol, labels, sizes, k, 3, EVERYTHING, 0) != vol).any()
    # a capacity below K: what is not known is not removed
    short = counts.copy()
    short[1] = k // 2
    want = select_np(vol, labels, sizes[:k // 2], k // 2, 3, EVERYTHING, 0)
    removed_all = select_np(vol, labels, sizes, k, 3, EVERYTHING, 0)
    assert (want != removed_all).any() and (want != vol).any()
    same(select(ctx, vol, labels, sizes[:k // 2], short, 3, EVERYTHING, 0, what="capacity below K"), want, "capacity below K")
    none = counts.copy()
    none[1] = 0
    same(select(ctx, vol, labels, sizes[:0], none, 3, EVERYTHING, 0, null_sizes=True, what="no sizes"), vol, "no sizes")
    # a box: its own labels; the bytes outside it untouched
    box = (40, 1, 2, 70, 5, 6)
    bl, bs, bc = check(ctx, vol, ISO, connectivity, box=box, what="labels of a box for select")
    want = select_np(vol, bl, bs[:int(bc[0])], int(bc[0]), 2, EVERYTHING, 3, box=box, dst=fresh)
    same(select(ctx, vol, bl, bs[:int(bc[0])], bc, 2, EVERYTHING, 3, box=box, what="box"), want, "box")
    want = select_np(vol, bl, bs[:int(bc[0])], int(bc[0]), 2, EVERYTHING, 3, box=box)
    same(select(ctx, vol, bl, bs[:int(bc[0])], bc, 2, EVERYTHING, 3, box=box, in_place=True, what="box, in place"), want, "box, in place")


# ---- Volume.label_components / remove_islands ---------------------------------------------------------------------------------------------
def test_volume_remove_islands_leaves_exactly_the_ball(ctx):
    clean = np.zeros((20, 20, 24), np.uint8)
    clean[4:16, 4:16, 6:18] = ball()
    vol = clean.copy()
    rng = np.random.default_rng(2)
    for z, y, x in ((1, 1, 1), (18, 18, 22), (1, 18, 3), (10, 1, 21), (18, 2, 12)):        # specks of 1 .. 8 voxels, away from the ball
        vol[z:z + 2, y:y + 2, x:x + 2] = np.where(rng.random((2, 2, 2)) < 0.6, 220, 0)
        vol[z, y, x] = 220
    ball_voxels = int((clean >= 128).sum())
    assert int((vol >= 128).sum()) > ball_voxels + 5
    v = make_volume(ctx, vol, block=2, packed=False)
    for use_max_map in (False, True):
        labels, sizes, counts = v.label_components(ISO, connectivity=6, use_max_map=use_max_map)
        wl, ws, wc = components_np(vol, ISO, 6)
        assert labels.dtype == torch.uint32 and sizes.dtype == torch.uint32 and tuple(labels.shape) == vol.shape
        same(labels.cpu().numpy(), wl, "Volume.label_components: labels")
        same(sizes.cpu().numpy(), ws, "Volume.label_components: sizes")
        assert counts.cpu().tolist() == wc.tolist() and wc[0] >= 6 and ws.max() == ball_voxels
    labels, sizes, counts = v.label_components(ISO, connectivity=26, sizes=False, box=((2, 3, 1), (17, 6, 9)))
    assert sizes is None and tuple(labels.shape) == (9, 6, 17)
    same(labels.cpu().numpy(), components_np(vol, ISO, 26, (2, 3, 1, 17, 6, 9))[0], "Volume.label_components: box")
    out = v.remove_islands(ISO, keep_largest=True)
    assert out.dtype == torch.uint8 and out.data_ptr() != v.volume.data_ptr()
    same(out.cpu().numpy(), clean, "remove_islands(keep_largest)")
    same(v.volume.cpu().numpy(), vol, "the volume itself")
    assert sorted(ws.tolist()) == [5, 5, 5, 5, 5, ball_voxels]
    same(v.remove_islands(ISO, min_voxels=6).cpu().numpy(), select_np(vol, wl, ws, len(ws), 6, EVERYTHING, 0), "remove_islands(min_voxels=6)")
    same(v.remove_islands(ISO, min_voxels=6).cpu().numpy(), clean, "remove_islands(min_voxels=6): the specks are gone")
    same(v.remove_islands(ISO, min_voxels=5).cpu().numpy(), vol, "remove_islands(min_voxels=5): specks of five voxels stay")
    # the mesh of the result is the oracle's mesh of the numpy-filtered volume: one closed shell
    filtered = make_volume(ctx, out.cpu().numpy(), block=2, packed=False)
    tri, total = filtered.extract_isosurface(ISO)
    assert total == len(mesh_np(clean, ISO)) == tuple(tri.shape)[0] and total < len(mesh_np(vol, ISO))
    target = torch.empty_like(v.volume)
    assert v.remove_islands(ISO, keep_largest=True, connectivity=26, fill=3, out=target) is target
    l26, s26, c26 = components_np(vol, ISO, 26)
    same(target.cpu().numpy(), select_np(vol, l26, s26, len(s26), int(s26.max()), EVERYTHING, 3), "remove_islands(keep_largest, 26, fill 3, out)")
    assert np.array_equal(l26 != 0, wl != 0) and (target.cpu().numpy()[(vol >= 128) & (clean < 128)] == 3).all()
    for kw in (dict(), dict(min_voxels=3, keep_largest=True), dict(min_voxels=-1), dict(min_voxels=3, fill=256), dict(min_voxels=3, connectivity=18)):
        with pytest.raises(ValueError):
            v.remove_islands(ISO, **kw)
    with pytest.raises(ValueError):
        v.label_components(ISO, box=((0, 0, 0), (25, 2, 2)))
