"""GPU: vkv_isosurface_mesh_indexed bit for bit against the numpy statement of tests/test_mesh_indexed_cpu.py (indexed_np):
the four counts, every vertex float, every normal float and every index, and against the device's own vkv_isosurface_mesh.

The kernels work in tiles of 256 x 4 VOXELS (four waves, each 64 lanes of four x-adjacent voxels of one row) that march over 16 slices; the
256 voxels of a wave are one ENTRY with a triangle count (the cubes that start there) and a vertex count (the crossing edges they own).  An
index needs the owner at x + 4, which is the lane above's first voxel and, for the last lane, the first voxel of the NEXT entry: widths 256,
257, 258 and 513 put the box's voxels at and just past one and two entries, where the segments of cubes and of owners part ways; the thin
extents exercise the far faces' owners and the narrow row path (W < 4).  2 x 66 x 65 crosses a scan chunk and 2 x 1026 x 1026 the 256 chunk
sums of one round, for each list.  Every buffer is a tests/helpers.py guarded() allocation, pre-filled and compared as a whole (an unwritten
element shows as the pre-fill, an element past the written count must still hold it), and all guards must be intact, so nothing here relies
on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_gpu_mesh import BOX_VOLUME, BOXES, FILL, ISO, block_extent, ext_of, sparse_volume, st
from tests.test_gpu_mesh import run as run_soup
from tests.test_gpu_mip import make_volume
from tests.test_mesh_cpu import MESH_CONTENTS, KINV255, ball, mesh_contents, mesh_np, same_bits
from tests.test_mesh_indexed_cpu import indexed_np, same_u32
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


def guard_damage(h):
    """Guarded.check() without a Python loop over the payload (the scratch of the largest case is 17 MB of non-fill bytes)"""
    changed = h.buf.cpu().numpy() != h.fill
    changed[h.start:h.stop] = False
    return np.flatnonzero(changed).tolist()


def run(ctx, vol, iso, cap_v, cap_t, box=None, block=0, vol_offset=0, vol_fill=0x00, normals=True, null_vertices=False, null_indices=False, map_extent=None,
        max_map=None, what=""):
    """(counts [4] uint64, the whole vertex buffer [cap_v, 3] float32, the whole normal buffer, the whole index buffer [cap_t, 3] uint32) of ONE
    vkv_isosurface_mesh_indexed call on guarded buffers, every output pre-filled with FILL; with `block` through the max map of that block size, with `map_extent` (w, h, d)
    through the map of that extent (built here, or the bytes `max_map`)"""
    abox = None if box is None else abi.Box(*box)
    d_vol, h_vol = T.guarded(vol, vol_offset, vol_fill, "cuda")
    nbytes = lib.mesh_indexed_scratch_bytes(ext_of(vol), abox)
    assert nbytes >= 16 and nbytes % 8 == 0, (what, nbytes)
    d_scratch, h_scratch = T.guarded((nbytes // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_counts, h_counts = T.guarded((4,), 0, FILL, "cuda", dtype=np.int64)
    d_vert, h_vert = T.guarded((max(cap_v, 1), 3), 0, FILL, "cuda", dtype=np.float32)
    d_norm, h_norm = T.guarded((max(cap_v, 1), 3), 0, FILL, "cuda", dtype=np.float32)
    d_idx, h_idx = T.guarded((max(cap_t, 1), 3), 0, FILL, "cuda", dtype=np.int32)
    handles = [("d_volume", h_vol), ("d_scratch", h_scratch), ("d_counts", h_counts), ("d_vertices", h_vert), ("d_normals", h_norm), ("d_indices", h_idx)]
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
    ctx.isosurface_mesh_indexed(d_vol.data_ptr(), ext_of(vol), abox, iso, None if d_map is None else d_map.data_ptr(), me, d_scratch.data_ptr(),
                                None if null_vertices else d_vert.data_ptr(), d_norm.data_ptr() if normals and not null_vertices else None, cap_v,
                                None if null_indices else d_idx.data_ptr(), cap_t, d_counts.data_ptr(), st())
    torch.cuda.synchronize()
    for name, h in handles:
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    assert np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    return d_counts.cpu().numpy().view(np.uint64), d_vert.cpu().numpy(), d_norm.cpu().numpy(), d_idx.cpu().numpy().view(np.uint32)


def prefilled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def check(ctx, vol, iso, want, cap_v=None, cap_t=None, normals=True, what="", **kw):
    """one call against the oracle's (vertices, normals, faces): the counts, the exact prefixes, the pre-fill behind them"""
    wv, wn, wf = want
    nv, nt = len(wv), len(wf)
    cap_v = nv + 5 if cap_v is None else cap_v
    cap_t = nt + 5 if cap_t is None else cap_t
    counts, vert, norm, idx = run(ctx, vol, iso, cap_v, cap_t, normals=normals, what=what, **kw)
    written_v, written_t = min(nv, cap_v), min(nt, cap_t)
    assert counts.tolist() == [nt, written_t, nv, written_v], "%s: counts %s, expected %s" % (what, counts.tolist(), [nt, written_t, nv, written_v])
    ev, en, ei = prefilled(vert.shape, np.float32), prefilled(norm.shape, np.float32), prefilled(idx.shape, np.uint32)
    ev[:written_v] = wv[:written_v]
    if normals:
        en[:written_v] = wn[:written_v]
    ei[:written_t] = wf[:written_t].astype(np.uint32)
    same_u32(vert, ev, what + ": vertices")
    same_u32(norm, en, what + ": normals")
    same_u32(idx, ei, what + ": indices")
    return counts, vert, norm, idx


# ---- extents and contents ---------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1, 1), (1, 4, 3), (2, 2, 2), (3, 1, 4), (4, 5, 1), (5, 4, 16), (6, 6, 17), (64, 2, 2), (65, 5, 3), (256, 4, 2), (257, 2, 17),
           (258, 6, 18), (513, 3, 3), (2, 66, 65)]  # (width, height, depth)


@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_and_content(ctx, extent):
    w, h, d = extent
    for k, content in enumerate(MESH_CONTENTS):
        vol = mesh_contents(content, (d, h, w), seed=700 + k)
        want = indexed_np(vol, ISO)
        what = "%s %s" % (content, extent)
        if content in ("below", "above") or min(extent) < 2:
            assert len(want[0]) == 0 and len(want[2]) == 0, what
        elif content != "ball" or min(extent) > 2:
            assert len(want[0]) > 0 and len(want[2]) > 0, what
        check(ctx, vol, ISO, want, what=what)


@pytest.mark.parametrize("extent", [(6, 6, 17), (257, 2, 17), (258, 6, 18), (513, 3, 3)], ids=lambda e: "%dx%dx%d" % e)
def test_against_the_devices_own_triangle_list(ctx, extent):
    w, h, d = extent
    vol = mesh_contents("random", (d, h, w), seed=31)
    soup_counts, tri = run_soup(ctx, vol, ISO, 12 * (w - 1) * (h - 1) * (d - 1), what="triangle list %s" % (extent,))
    total = int(soup_counts[0])
    assert total > 0 and soup_counts[1] == total
    counts, vert, _, idx = run(ctx, vol, ISO, 7 * w * h * d, total, what="indexed %s" % (extent,))
    assert counts[0] == total == counts[1] and counts[2] == counts[3] > 0
    assert idx[:total].max() == counts[2] - 1
    same_bits(vert[idx[:total].astype(np.int64)], tri[:total], "vertices[indices] %s" % (extent,))


@pytest.fixture(scope="module")
def rounds_case():
    """2 x 1026 x 1026: 1026 x 1026 entries = 257 chunks of 4096 for each list, so the workgroup that scans a list's chunk sums carries a total
    into a second round; five bright rows far apart"""
    w, h, d = 2, 1026, 1026
    vol = np.zeros((d, h, w), np.uint8)
    for z, y in ((0, 0), (3, 1000), (512, 513), (1023, 0), (1025, 1025)):
        vol[z, y, :] = 255
    want = indexed_np(vol, ISO)
    assert len(want[0]) > 0 and len(want[2]) > 0
    return vol, want


@pytest.mark.parametrize("short", ["full", "vertices - 1", "triangles - 1"])
def test_more_chunk_sums_than_one_round_of_the_scan(ctx, rounds_case, short):
    vol, want = rounds_case
    nv, nt = len(want[0]), len(want[2])
    check(ctx, vol, ISO, want, cap_v=nv - 1 if short == "vertices - 1" else nv, cap_t=nt - 1 if short == "triangles - 1" else nt, what="257 chunks, " + short)


# ---- alignment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(7, 3, 3), (261, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_volume_alignment_with_both_guard_fills(ctx, extent):
    """odd widths: a row's tail and the next row's head share a dword, and the last row ends where the guard begins; a result that consumed a
    guard byte (as a voxel or as a normal's neighbour) differs under one of the two fills"""
    w, h, d = extent
    vol = mesh_contents("random", (d, h, w), seed=77)
    want = indexed_np(vol, ISO)
    for fill in (0x00, 0xFF):
        for offset in (0, 1, 2, 3, 5, 7):
            check(ctx, vol, ISO, want, vol_offset=offset, vol_fill=fill, what="%s volume +%d fill %#x" % (extent, offset, fill))


# ---- capacities -------------------------------------------------------------------------------------------------------------------------
def test_capacities_give_exact_prefixes_full_totals_and_the_same_indices(ctx):
    vol = mesh_contents("random", (18, 6, 70), seed=3)
    want = indexed_np(vol, ISO)
    nv, nt = len(want[0]), len(want[2])
    assert nv > 1000 and nt > 1000
    for cap_v, cap_t in ((1, nt), (7, nt + 5), (nv - 1, nt), (nv, 1), (nv + 5, 7), (nv, nt - 1), (nv, nt), (3, 5)):
        check(ctx, vol, ISO, want, cap_v=cap_v, cap_t=cap_t, what="capacities %d of %d vertices, %d of %d triangles" % (cap_v, nv, cap_t, nt))
    counts, vert, norm, idx = run(ctx, vol, ISO, 0, 0, null_vertices=True, null_indices=True, what="counting call")
    assert counts.tolist() == [nt, 0, nv, 0]
    assert all((a.view(np.uint8) == FILL).all() for a in (vert, norm, idx))
    check(ctx, vol, ISO, want, cap_v=0, cap_t=0, normals=False, what="both capacities 0 with buffers")
    counts, vert, norm, idx = run(ctx, vol, ISO, nv, 0, null_indices=True, what="vertices only")
    assert counts.tolist() == [nt, 0, nv, nv] and (idx.view(np.uint8) == FILL).all()
    same_u32(vert, want[0], "vertices only")
    same_u32(norm, want[1], "vertices only: normals")
    counts, vert, norm, idx = run(ctx, vol, ISO, 0, nt, null_vertices=True, what="indices only")
    assert counts.tolist() == [nt, nt, nv, 0] and (vert.view(np.uint8) == FILL).all() and (norm.view(np.uint8) == FILL).all()
    same_u32(idx, want[2].astype(np.uint32), "indices only")
    check(ctx, vol, ISO, want, normals=False, what="normals NULL")        # the normal buffer keeps its pre-fill
    check(ctx, vol, ISO, want, normals=False, cap_v=nv - 3, what="normals NULL, vertices short")


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
MORE_BOXES = {"far corner, wide": (40, 2, 3, 261, 7, 17), "far face x, two entries": (44, 1, 1, 257, 3, 3), "height 1 inside": (7, 4, 2, 9, 1, 5)}


@pytest.fixture(scope="module")
def box_volume():
    w, h, d = BOX_VOLUME
    return mesh_contents("random", (d, h, w), seed=91)


@pytest.mark.parametrize("box", sorted(BOXES) + sorted(MORE_BOXES), ids=lambda b: b.replace(" ", "_").replace(",", ""))
def test_a_box_gives_its_own_edges_with_the_whole_volumes_normals(ctx, box_volume, box):
    b = BOXES.get(box) or MORE_BOXES[box]
    want = indexed_np(box_volume, ISO, b)
    if min(b[3:]) < 2:
        assert len(want[0]) == 0 and len(want[2]) == 0
    else:
        assert len(want[0]) > 0 and len(want[2]) > 0
    check(ctx, box_volume, ISO, want, box=b, what="box %s" % box)
    check(ctx, box_volume, ISO, want, box=b, block=4, what="box %s, max map" % box)


# ---- max map ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [2, 4])
def test_max_map_gives_the_dense_bytes(ctx, block):
    vol = sparse_volume()
    want = indexed_np(vol, ISO)
    assert len(want[2]) > 100
    dense = check(ctx, vol, ISO, want, what="dense")
    sparse = check(ctx, vol, ISO, want, block=block, what="max map, block %d" % block)
    for a, b in zip(dense, sparse):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    check(ctx, vol, ISO, want, block=block, cap_v=len(want[0]) // 2, cap_t=len(want[2]) // 3, what="max map, block %d, short capacities" % block)
    check(ctx, vol, 0.05, indexed_np(vol, 0.05), block=block, what="max map, block %d, iso 0.05: nothing skipped" % block)
    empty = indexed_np(vol, 1.5)
    assert len(empty[0]) == 0
    check(ctx, vol, 1.5, empty, block=block, what="max map, block %d, nothing inside" % block)


def test_iso_on_a_voxel_value_keeps_the_coincident_vertices(ctx):
    iso = np.float32(128) * KINV255
    vol = np.random.default_rng(6).integers(120, 137, size=(5, 6, 9), dtype=np.uint8)
    vol[1:3, 2, 3:6] = 128
    want = indexed_np(vol, iso)
    assert len(np.unique(want[0].view(np.uint32), axis=0)) < len(want[0])        # several edges, one position
    check(ctx, vol, float(iso), want, what="iso = 128 / 255")
    check(ctx, vol, float(iso), want, block=2, what="iso = 128 / 255, max map")


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(ctx):
    vol = mesh_contents("random", (19, 5, 258), seed=21)
    want = indexed_np(vol, ISO)
    a = check(ctx, vol, ISO, want, what="first run")
    b = check(ctx, vol, ISO, want, what="second run")
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_one_call_captured_into_a_graph_replays(ctx):
    shape = (17, 9, 131)
    vol = mesh_contents("random", shape, seed=13)
    cap_v, cap_t = 7 * 17 * 9 * 131, 12 * 16 * 8 * 130
    d_vol = torch.from_numpy(vol).cuda()
    d_scratch = torch.empty((lib.mesh_indexed_scratch_bytes(ext_of(vol)) // 8,), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros((4,), dtype=torch.int64, device="cuda")
    d_vert = torch.empty((cap_v, 3), dtype=torch.float32, device="cuda")
    d_norm = torch.empty((cap_v, 3), dtype=torch.float32, device="cuda")
    d_idx = torch.empty((cap_t, 3), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def call():
        ctx.isosurface_mesh_indexed(d_vol.data_ptr(), ext_of(vol), None, ISO, None, None, d_scratch.data_ptr(), d_vert.data_ptr(), d_norm.data_ptr(), cap_v,
                                    d_idx.data_ptr(), cap_t, d_counts.data_ptr(), s.cuda_stream)

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
        for t in (d_vert, d_norm, d_idx):
            t.view(torch.uint8).fill_(FILL)
        d_counts.fill_(-1)
        d_scratch.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        wv, wn, wf = indexed_np(vol, ISO)
        assert d_counts.cpu().tolist() == [len(wf), len(wf), len(wv), len(wv)] and len(wv) <= cap_v and len(wf) <= cap_t
        same_u32(d_vert[:len(wv)].cpu().numpy(), wv, "replay, seed %d: vertices" % seed)
        same_u32(d_norm[:len(wv)].cpu().numpy(), wn, "replay, seed %d: normals" % seed)
        same_u32(d_idx[:len(wf)].cpu().numpy().view(np.uint32), wf.astype(np.uint32), "replay, seed %d: indices" % seed)
        assert all(bool((t[n:].view(torch.uint8) == FILL).all()) for t, n in ((d_vert, len(wv)), (d_norm, len(wv)), (d_idx, len(wf))))


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")        # [scratch 2048 | counts 32 | vertices 2016 | normals 2048 | indices 2048]
    a = out.data_ptr()
    assert a % 8 == 0 and lib.mesh_indexed_scratch_bytes(e) <= 2048
    scratch, counts, vert, norm, idx, v = a, a + 2048, a + 2080, a + 4096, a + 6144, vol.data_ptr()
    me, none = abi.Extent3D(3, 2, 1), None
    bad, inf, nan = abi.VKV_E_INVALID_ARGUMENT, float("inf"), float("nan")
    rc = lambda *args: ctx.isosurface_mesh_indexed_rc(*args, st())  # noqa: E731
    tail = (scratch, vert, norm, 10, idx, 10, counts)
    assert rc(None, e, None, 0.5, None, none, *tail) == bad
    assert rc(v, e, None, 0.5, None, none, None, vert, norm, 10, idx, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, vert, norm, 10, idx, 10, None) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, None, None, 10, idx, 10, counts) == bad and "d_vertices" in ctx.last_error()
    assert rc(v, e, None, 0.5, None, none, scratch, None, norm, 10, idx, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, vert, norm, 10, None, 10, counts) == bad and "d_indices" in ctx.last_error()
    assert rc(v, e, None, 0.5, None, none, scratch, None, norm, 0, idx, 10, counts) == bad and "d_normals" in ctx.last_error()
    assert rc(v, e, None, 0.5, None, none, scratch, vert, norm, 0, idx, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, vert, norm, 1 << 32, idx, 10, counts) == bad and "32-bit" in ctx.last_error()
    assert rc(v, abi.Extent3D(w, 0, d), None, 0.5, None, none, *tail) == bad
    for iso in (inf, -inf, nan):
        assert rc(v, e, None, iso, None, none, *tail) == bad and "iso" in ctx.last_error()
    assert rc(v, e, abi.Box(0, 0, 0, 13, 2, 2), 0.5, None, none, *tail) == bad and "box" in ctx.last_error()
    assert rc(v, e, abi.Box(11, 4, 3, 1, 2, 1), 0.5, None, none, *tail) == bad
    assert rc(v, e, abi.Box(1, 1, 1, 2, 0, 2), 0.5, None, none, *tail) == bad
    assert rc(v, e, None, 0.5, v, none, *tail) == bad and "map_extent" in ctx.last_error()
    assert rc(v, e, None, 0.5, v, abi.Extent3D(13, 2, 1), *tail) == bad
    assert rc(v, e, None, 0.5, None, none, scratch + 4, vert, norm, 10, idx, 10, counts) == bad and "aligned" in ctx.last_error()
    assert rc(v, e, None, 0.5, None, none, scratch, vert + 2, norm, 10, idx, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, vert, norm + 1, 10, idx, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, vert, norm, 10, idx + 2, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, vert, norm, 10, idx, 10, counts + 4) == bad
    assert rc(v, abi.Extent3D(0x80000000, 2, 2), None, 0.5, None, none, *tail) == abi.VKV_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # and the accepted call next to them, with a valid max map argument that is not used: a volume without a surface
    assert rc(v, e, None, 0.5, None, me, *tail) == abi.VKV_OK
    torch.cuda.synchronize()
    assert out[2048:2080].view(torch.int64).tolist() == [0, 0, 0, 0] and bool((out[2080:] == FILL).all())


# ---- Volume.extract_isosurface_indexed ---------------------------------------------------------------------------------------------------
def test_volume_extract_isosurface_indexed_matches_the_c_call(ctx):
    vol = ball()
    wv, wn, wf = indexed_np(vol, ISO)
    assert (len(wv), len(wf)) == (914, 1824)
    counts, c_vert, c_norm, c_idx = run(ctx, vol, ISO, 914, 1824, what="C call")
    assert counts.tolist() == [1824, 1824, 914, 914]
    v = make_volume(ctx, vol, block=2, packed=False)
    for use_max_map in (False, True):
        vertices, faces, normals = v.extract_isosurface_indexed(ISO, normals=True, use_max_map=use_max_map)
        assert tuple(vertices.shape) == (914, 3) and tuple(faces.shape) == (1824, 3) and tuple(normals.shape) == (914, 3)
        assert vertices.dtype == torch.float32 and faces.dtype == torch.uint32 and normals.dtype == torch.float32
        same_u32(vertices.cpu().numpy(), c_vert, "extract_isosurface_indexed: vertices")
        same_u32(normals.cpu().numpy(), c_norm, "extract_isosurface_indexed: normals")
        same_u32(faces.cpu().numpy(), c_idx, "extract_isosurface_indexed: faces")
    vertices, faces, normals = v.extract_isosurface_indexed(ISO)
    assert normals is None
    same_u32(vertices.cpu().numpy(), wv, "no normals")
    tri, total = v.extract_isosurface(ISO)
    same_bits(vertices.cpu().numpy()[faces.cpu().numpy().astype(np.int64)], tri.cpu().numpy(), "against extract_isosurface")
    vertices, faces, normals, counts = v.extract_isosurface_indexed(ISO, capacity=(500, 1000), normals=True, use_max_map=True)
    assert tuple(vertices.shape) == (500, 3) and tuple(faces.shape) == (1000, 3) and counts.cpu().tolist() == [1824, 1000, 914, 500]
    same_u32(vertices.cpu().numpy(), wv[:500], "capacity: vertices")
    same_u32(normals.cpu().numpy(), wn[:500], "capacity: normals")
    same_u32(faces.cpu().numpy(), wf[:1000].astype(np.uint32), "capacity: faces")
    vertices, faces, normals, counts = v.extract_isosurface_indexed(ISO, capacity=(0, 0))
    assert tuple(vertices.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and normals is None and counts.cpu().tolist() == [1824, 0, 914, 0]
    box = ((2, 3, 1), (7, 6, 9))
    vertices, faces, normals = v.extract_isosurface_indexed(ISO, box=box, normals=True)
    bv, bn, bf = indexed_np(vol, ISO, (2, 3, 1, 7, 6, 9))
    assert len(bv) > 0
    same_u32(vertices.cpu().numpy(), bv, "box: vertices")
    same_u32(normals.cpu().numpy(), bn, "box: normals")
    same_u32(faces.cpu().numpy(), bf.astype(np.uint32), "box: faces")
    vertices, faces, normals = v.extract_isosurface_indexed(1.5, normals=True)
    assert tuple(vertices.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and tuple(normals.shape) == (0, 3)
    with pytest.raises(ValueError):
        v.extract_isosurface_indexed(ISO, box=((0, 0, 0), (13, 2, 2)))
    with pytest.raises(ValueError):
        v.extract_isosurface_indexed(ISO, capacity=(1 << 32, 1))
