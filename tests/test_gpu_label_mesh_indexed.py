"""GPU: vkv_label_mesh_indexed bit for bit against the numpy statement of tests/test_label_mesh_indexed_cpu.py
(label_indexed_np): the four counts, every vertex float, every normal float, every label pair, every index and every triangle label; and
against the device's own vkv_label_mesh and vkv_isosurface_mesh_indexed.

The kernels work in the tiles of vkv_isosurface_mesh_indexed: 256 x 4 VOXELS (four waves, each 64 lanes of four x-adjacent voxels of one row)
that march over 16 slices; the 256 voxels of a wave are one ENTRY with a triangle count (the cubes that start there) and a vertex count (the
crossing edges they own).  An index needs the owner at x + 4, which is the lane above's first voxel and, for the last lane, the first voxel of
the NEXT entry: widths 256, 257, 258 and 513 put the box's voxels at and just past one and two entries, where the segments of cubes and of
owners part ways; the thin extents exercise the far faces' owners and the narrow row path (W < 4).  Every voxel's crossing mask is one byte of
scratch in rows rounded up to four, so widths 1 .. 7 and 257 .. 261 also walk that padding.  2 x 66 x 65 crosses a scan chunk and 2 x 1026 x
1026 the 256 chunk sums of one round, for each list.  Every buffer is a tests/helpers.py guarded() allocation, pre-filled and compared as a
whole (an unwritten element shows as the pre-fill, an element past the written count must still hold it), and all guards must be intact, so
nothing here relies on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_gpu_label_mesh import run as run_list
from tests.test_gpu_mesh import BOX_VOLUME, BOXES
from tests.test_gpu_mesh_indexed import MORE_BOXES
from tests.test_gpu_mesh_indexed import run as run_iso_indexed
from tests.test_gpu_mip import make_volume
from tests.test_label_mesh_cpu import SKIP_COLORS, SKIP_SHAPE, bordered, distinct_labels, random_labels, rounds_labels, skip_labels
from tests.test_label_mesh_indexed_cpu import label_indexed_np
from tests.test_labels_render_cpu import visibility_map_np
from tests.test_mesh_cpu import mesh_contents, same_bits
from tests.test_mesh_indexed_cpu import same_u32
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


def guard_damage(h):
    """Guarded.check() without a Python loop over the payload (the scratch of the largest case is 21 MB of non-fill bytes)"""
    changed = h.buf.cpu().numpy() != h.fill
    changed[h.start:h.stop] = False
    return np.flatnonzero(changed).tolist()


def run(ctx, labels, cap_v, cap_t, colors=None, vol=None, iso=None, box=None, shape=None, map_extent=None, label_offset=0, label_fill=0x00, vol_offset=0,
        vol_fill=0x00, normals=None, pairs=True, null_vertices=False, null_indices=False, what=""):
    """(counts [4] uint64, and the whole buffers: vertices [cap_v, 3] float32, normals [cap_v, 3] float32, label pairs [cap_v, 2] uint32, indices
    [cap_t, 3] uint32, triangle labels [cap_t] uint32) of ONE vkv_label_mesh_indexed call on guarded buffers, every output pre-filled with
    FILL.  labels: the box's shape; shape: the volume's (d, h, w) (None: the labels' or the volume's own); normals None: asked for with a
    volume; map_extent (w, h, d): through vkv_label_visibility_map of that extent, built here"""
    shape = (vol.shape if vol is not None else labels.shape) if shape is None else shape
    normals = vol is not None if normals is None else normals
    e = ext_of(shape)
    abox = None if box is None else abi.Box(*box)
    d_lab, h_lab = T.guarded(labels.view(np.int32), label_offset, label_fill, "cuda")
    handles = [("d_labels", h_lab)]
    d_col = d_vol = d_map = me = None
    if colors is not None:
        d_col, h_col = T.guarded(np.asarray(colors, np.uint32).view(np.int32), 0, 0xFF, "cuda")
        handles.append(("d_colors", h_col))
    if vol is not None:
        d_vol, h_vol = T.guarded(vol, vol_offset, vol_fill, "cuda")
        handles.append(("d_volume", h_vol))
    nbytes = LB.mesh_indexed_scratch_bytes(e, abox)
    assert nbytes >= 16 and nbytes % 8 == 0, (what, nbytes)
    d_scratch, h_scratch = T.guarded((nbytes // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_counts, h_counts = T.guarded((4,), 0, FILL, "cuda", dtype=np.int64)
    d_vert, h_vert = T.guarded((max(cap_v, 1), 3), 0, FILL, "cuda", dtype=np.float32)
    d_norm, h_norm = T.guarded((max(cap_v, 1), 3), 0, FILL, "cuda", dtype=np.float32)
    d_pair, h_pair = T.guarded((max(cap_v, 1), 2), 0, FILL, "cuda", dtype=np.int32)
    d_idx, h_idx = T.guarded((max(cap_t, 1), 3), 0, FILL, "cuda", dtype=np.int32)
    d_tl, h_tl = T.guarded((max(cap_t, 1),), 0, FILL, "cuda", dtype=np.int32)
    handles += [("d_scratch", h_scratch), ("d_counts", h_counts), ("d_vertices", h_vert), ("d_normals", h_norm), ("d_vertex_labels", h_pair),
                ("d_indices", h_idx), ("d_triangle_labels", h_tl)]
    if map_extent is not None:
        me = abi.Extent3D(*map_extent)
        d_map, h_map = T.guarded((me.depth, me.height, me.width), 0, FILL, "cuda")
        handles.append(("d_visibility_map", h_map))
        ctx.check(ctx.label_visibility_map_rc(d_lab.data_ptr(), e, abox, d_col.data_ptr(), len(colors), me, d_map.data_ptr(), st()))
    ctx.check(ctx.label_mesh_indexed_rc(
        d_lab.data_ptr(), e, abox, None if d_col is None else d_col.data_ptr(), 0 if colors is None else len(colors), None if d_vol is None else d_vol.data_ptr(),
        0.0 if iso is None else iso, None if d_map is None else d_map.data_ptr(), me, d_scratch.data_ptr(), None if null_vertices else d_vert.data_ptr(),
        d_norm.data_ptr() if normals and not null_vertices else None, d_pair.data_ptr() if pairs and not null_vertices else None, cap_v,
        None if null_indices else d_idx.data_ptr(), None if null_indices else d_tl.data_ptr(), cap_t, d_counts.data_ptr(), st()))
    torch.cuda.synchronize()
    for name, h in handles:
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    assert np.array_equal(d_lab.cpu().numpy().view(np.uint32), labels), "%s: the labels changed" % what
    assert vol is None or np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    return (d_counts.cpu().numpy().view(np.uint64), d_vert.cpu().numpy(), d_norm.cpu().numpy(), d_pair.cpu().numpy().view(np.uint32),
            d_idx.cpu().numpy().view(np.uint32), d_tl.cpu().numpy().view(np.uint32))


def prefilled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def check(ctx, labels, want, cap_v=None, cap_t=None, normals=None, pairs=True, what="", **kw):
    """one call against the oracle's (vertices, normals, pairs, faces, face labels): the counts, the exact prefixes, the pre-fill behind them"""
    wv, wn, wp, wf, wl = want
    nv, nt = len(wv), len(wf)
    cap_v = nv + 5 if cap_v is None else cap_v
    cap_t = nt + 5 if cap_t is None else cap_t
    normals = wn is not None if normals is None else normals
    counts, vert, norm, pair, idx, tl = got = run(ctx, labels, cap_v, cap_t, normals=normals, pairs=pairs, what=what, **kw)
    written_v, written_t = min(nv, cap_v), min(nt, cap_t)
    assert counts.tolist() == [nt, written_t, nv, written_v], "%s: counts %s, expected %s" % (what, counts.tolist(), [nt, written_t, nv, written_v])
    ev, en, ep = prefilled(vert.shape, np.float32), prefilled(norm.shape, np.float32), prefilled(pair.shape, np.uint32)
    ei, el = prefilled(idx.shape, np.uint32), prefilled(tl.shape, np.uint32)
    ev[:written_v] = wv[:written_v]
    if normals:
        en[:written_v] = wn[:written_v]
    if pairs:
        ep[:written_v] = wp[:written_v]
    ei[:written_t] = wf[:written_t].astype(np.uint32)
    el[:written_t] = wl[:written_t]
    same_u32(vert, ev, what + ": vertices")
    same_u32(norm, en, what + ": normals")
    same_u32(pair, ep, what + ": vertex labels")
    same_u32(idx, ei, what + ": indices")
    same_u32(tl, el, what + ": triangle labels")
    return got


def table_for(labels):
    """a table that hides label 1 and ends one below the largest label"""
    return LB.color_table(max(int(labels.max()) - 1, 1), seed=4, hidden=(1,))


# ---- extents and contents ---------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1, 1), (1, 4, 3), (2, 2, 2), (3, 1, 4), (4, 5, 1), (5, 4, 16), (6, 6, 17), (64, 2, 2), (65, 5, 3), (256, 4, 2), (257, 2, 17),
           (258, 6, 18), (513, 3, 3), (2, 66, 65)]  # (width, height, depth)


@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_and_content(ctx, extent):
    w, h, d = extent
    shape = (d, h, w)
    cubes = (w - 1) * (h - 1) * (d - 1)
    vol = mesh_contents("random", shape, seed=900 + w)
    high = (128 + vol // 2).astype(np.uint8)        # every byte at or above iso 0.5: nothing crosses, every t = 0.5f, the normals are not zero
    contents = {
        "zeros": (np.zeros(shape, np.uint32), vol),
        "one label": (np.full(shape, 7, np.uint32), vol),
        "random": (random_labels(shape, 800 + w, top=3), vol),
        "distinct": (distinct_labels(shape), vol),        # every tetrahedron pattern 1 + 1 + 1 + 1, 24 triangles per cube
        "two labels": (2 + random_labels(shape, 850 + w, top=1), high),        # no zero: interfaces only
    }
    for name, (labels, v) in contents.items():
        for colors in (None, table_for(labels)):
            for with_volume in (False, True):
                what = "%s %s%s%s" % (name, extent, ", table" if colors is not None else "", ", volume" if with_volume else "")
                want = label_indexed_np(labels, colors, v if with_volume else None, ISO if with_volume else None)
                if name in ("zeros", "one label") or cubes == 0:
                    assert len(want[0]) == 0 and len(want[3]) == 0, what
                elif colors is None:
                    assert len(want[0]) > 0 and len(want[3]) > 0, what
                if name == "distinct" and colors is None:
                    assert len(want[3]) == 24 * cubes, what
                if name == "two labels" and with_volume and len(want[0]):
                    frac = want[0] % 1
                    assert np.isin(frac, (0.0, 0.5)).all() and ((frac == 0.5).sum(axis=1) >= 1).all(), what        # every t = 0.5f
                    assert (want[1] != 0).any(), what
                check(ctx, labels, want, colors=colors, vol=v if with_volume else None, iso=ISO if with_volume else None, what=what)


@pytest.fixture(scope="module")
def rounds_case():
    """2 x 1026 x 1026: 1026 x 1026 entries = 257 chunks of 4096 for each list, so the workgroup that scans a list's chunk sums carries a total
    into a second round; five labelled rows far apart"""
    labels = rounds_labels()
    want = label_indexed_np(labels)
    assert len(want[0]) > 0 and len(want[3]) > 0 and sorted(set(want[4].tolist())) == [1, 2, 3]
    return labels, want


@pytest.mark.parametrize("short", ["full", "vertices - 1", "triangles - 1"])
def test_more_chunk_sums_than_one_round_of_the_scan(ctx, rounds_case, short):
    labels, want = rounds_case
    nv, nt = len(want[0]), len(want[3])
    check(ctx, labels, want, cap_v=nv - 1 if short == "vertices - 1" else nv, cap_t=nt - 1 if short == "triangles - 1" else nt, what="257 chunks, " + short)


# ---- against the device's own calls -------------------------------------------------------------------------------------------------------
FOUR = [(6, 6, 17), (257, 2, 17), (258, 6, 18), (513, 3, 3)]


@pytest.mark.parametrize("extent", FOUR, ids=lambda e: "%dx%dx%d" % e)
def test_against_the_devices_own_triangle_list(ctx, extent):
    w, h, d = extent
    labels = random_labels((d, h, w), 31, top=4)
    vol = mesh_contents("random", (d, h, w), seed=32)
    colors = LB.color_table(3, hidden=(2,))
    cap = 24 * (w - 1) * (h - 1) * (d - 1)
    list_counts, tri, tri_labels = run_list(ctx, labels, colors=colors, vol=vol, iso=ISO, capacity=cap, what="triangle list %s" % (extent,))
    total = int(list_counts[0])
    assert total > 0 and list_counts[1] == total
    counts, vert, _, pair, idx, tl = run(ctx, labels, 7 * w * h * d, total, colors=colors, vol=vol, iso=ISO, what="indexed %s" % (extent,))
    assert counts[0] == total == counts[1] and counts[2] == counts[3] > 0
    assert idx[:total].max() == counts[2] - 1 and len(np.unique(idx[:total])) == counts[2]        # no orphans
    same_bits(vert[idx[:total].astype(np.int64)], tri[:total], "vertices[indices] %s" % (extent,))
    assert np.array_equal(tl[:total], tri_labels[:total])
    assert (pair[idx[:total].astype(np.int64)] == tl[:total, None, None]).any(axis=2).all()


@pytest.mark.parametrize("extent", FOUR, ids=lambda e: "%dx%dx%d" % e)
def test_against_the_devices_own_indexed_isosurface_on_the_14_components(ctx, extent):
    w, h, d = extent
    iso = 0.8
    vol = mesh_contents("random", (d, h, w), seed=33)
    v = make_volume(ctx, vol, block=2, packed=False)
    labels = v.label_components(iso, connectivity=14, sizes=False)[0].cpu().numpy().view(np.uint32)
    assert labels.max() > 3
    cap_v, cap_t = 7 * w * h * d, 12 * (w - 1) * (h - 1) * (d - 1)
    want_counts, want_vert, want_norm, want_idx = run_iso_indexed(ctx, vol, iso, cap_v, cap_t, what="isosurface_mesh_indexed %s" % (extent,))
    counts, vert, norm, pair, idx, tl = run(ctx, labels, cap_v, cap_t, vol=vol, iso=iso, what="label_mesh_indexed %s" % (extent,))
    assert counts.tolist() == want_counts.tolist() and counts[0] == counts[1] > 0 and counts[2] == counts[3] > 0
    same_u32(vert, want_vert, "vertices %s" % (extent,))
    same_u32(norm, want_norm, "normals %s" % (extent,))
    same_u32(idx, want_idx, "indices %s" % (extent,))
    nv = int(counts[2])
    assert (pair[:nv].min(axis=1) == 0).all() and (pair[:nv].max(axis=1) >= 1).all()        # a body against nothing, everywhere


# ---- alignment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(7, 3, 3), (261, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_label_and_volume_alignment_with_both_guard_fills(ctx, extent):
    """odd widths: a row's tail and the next row's head share a load, and the last row ends where the guard begins; a result that consumed a
    guard label or byte (as a voxel or as a normal's neighbour) differs under one of the two fills"""
    w, h, d = extent
    labels = random_labels((d, h, w), 77)
    vol = mesh_contents("random", (d, h, w), seed=78)
    want = label_indexed_np(labels, None, vol, ISO)
    for fill in (0x00, 0xFF):
        for k, vol_offset in enumerate((0, 1, 2, 3, 5, 7)):
            offset = 4 * (k % 4)
            check(ctx, labels, want, vol=vol, iso=ISO, label_offset=offset, label_fill=fill, vol_offset=vol_offset, vol_fill=fill,
                  what="%s labels +%d volume +%d fill %#x" % (extent, offset, vol_offset, fill))


# ---- capacities -------------------------------------------------------------------------------------------------------------------------
def test_capacities_give_exact_prefixes_full_totals_and_the_same_indices(ctx):
    labels = random_labels((18, 6, 70), 3)
    vol = mesh_contents("random", (18, 6, 70), seed=4)
    want = label_indexed_np(labels, None, vol, ISO)
    nv, nt = len(want[0]), len(want[3])
    assert nv > 1000 and nt > 1000
    kw = dict(vol=vol, iso=ISO)
    for cap_v, cap_t in ((1, nt), (7, nt + 5), (nv - 1, nt), (nv, 1), (nv + 5, 7), (nv, nt - 1), (nv, nt), (3, 5)):
        check(ctx, labels, want, cap_v=cap_v, cap_t=cap_t, what="capacities %d of %d vertices, %d of %d triangles" % (cap_v, nv, cap_t, nt), **kw)
    got = run(ctx, labels, 0, 0, null_vertices=True, null_indices=True, what="counting call", **kw)
    assert got[0].tolist() == [nt, 0, nv, 0]
    assert all((a.view(np.uint8) == FILL).all() for a in got[1:])
    check(ctx, labels, want, cap_v=0, cap_t=0, normals=False, pairs=False, what="both capacities 0 with buffers", **kw)
    counts, vert, norm, pair, idx, tl = run(ctx, labels, nv, 0, null_indices=True, what="vertices only", **kw)
    assert counts.tolist() == [nt, 0, nv, nv] and (idx.view(np.uint8) == FILL).all() and (tl.view(np.uint8) == FILL).all()
    same_u32(vert, want[0], "vertices only")
    same_u32(norm, want[1], "vertices only: normals")
    same_u32(pair, want[2], "vertices only: vertex labels")
    counts, vert, norm, pair, idx, tl = run(ctx, labels, 0, nt, null_vertices=True, what="indices only", **kw)
    assert counts.tolist() == [nt, nt, nv, 0] and all((a.view(np.uint8) == FILL).all() for a in (vert, norm, pair))
    same_u32(idx, want[3].astype(np.uint32), "indices only")
    same_u32(tl, want[4], "indices only: triangle labels")
    check(ctx, labels, want, normals=False, what="normals NULL", **kw)        # the normal buffer keeps its pre-fill
    check(ctx, labels, want, pairs=False, what="vertex labels NULL", **kw)
    check(ctx, labels, want, normals=False, pairs=False, cap_v=nv - 3, what="normals and vertex labels NULL, vertices short", **kw)


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box_volume():
    w, h, d = BOX_VOLUME
    return mesh_contents("random", (d, h, w), seed=91)


@pytest.mark.parametrize("box", sorted(BOXES) + sorted(MORE_BOXES), ids=lambda b: b.replace(" ", "_").replace(",", ""))
def test_a_box_takes_labels_of_its_shape_and_the_whole_volumes_normals(ctx, box_volume, box):
    w, h, d = BOX_VOLUME
    b = BOXES.get(box) or MORE_BOXES[box]
    labels = random_labels((b[5], b[4], b[3]), 92, top=4)
    colors = LB.color_table(4, hidden=(3,))
    want = label_indexed_np(labels, colors, box_volume, ISO, b)
    assert (len(want[0]) > 0) == (min(b[3:]) > 1) and (len(want[3]) > 0) == (min(b[3:]) > 1)
    check(ctx, labels, want, colors=colors, vol=box_volume, iso=ISO, box=b, what="box %s" % box)
    check(ctx, labels, want, colors=colors, vol=box_volume, iso=ISO, box=b, map_extent=((w + 3) // 4, (h + 3) // 4, (d + 3) // 4), what="box %s, map" % box)
    check(ctx, labels, label_indexed_np(labels, colors, box=b), colors=colors, shape=(d, h, w), box=b, what="box %s, midpoints" % box)


# ---- visibility map -----------------------------------------------------------------------------------------------------------------------
def empty_voxel_tiles(vis_map, shape_dhw, map_extent):
    """the tiles of 256 x 4 x 16 VOXELS of the whole volume all of whose voxels lie in cells that hold 0 (the kernels' test), of how many"""
    D, H, W = shape_dhw
    mw, mh, md = map_extent
    bx, by, bz = -(-W // mw), -(-H // mh), -(-D // md)
    empty = total = 0
    for zt in range(0, D, 16):
        for yt in range(0, H, 4):
            for xt in range(0, W, 256):
                cells = vis_map[zt // bz:(min(zt + 16, D) - 1) // bz + 1, yt // by:(min(yt + 4, H) - 1) // by + 1, xt // bx:(min(xt + 256, W) - 1) // bx + 1]
                total += 1
                empty += int(not cells.any())
    return empty, total


@pytest.fixture(scope="module")
def skip_scene():
    labels = skip_labels()
    vol = mesh_contents("random", SKIP_SHAPE, seed=33)
    return labels, vol, label_indexed_np(labels, SKIP_COLORS), label_indexed_np(labels, SKIP_COLORS, vol, ISO)


@pytest.mark.parametrize("map_extent", [(300, 9, 20), (75, 3, 5), (38, 9, 4)], ids=["block1", "block4", "8x1x5"])
def test_visibility_map_gives_the_dense_bits(ctx, skip_scene, map_extent):
    labels, vol, want_mid, want_vol = skip_scene
    vis = visibility_map_np(labels, None, SKIP_SHAPE, SKIP_COLORS, map_extent)
    empty, total = empty_voxel_tiles(vis, SKIP_SHAPE, map_extent)
    assert total == 2 * 3 * 2 and empty >= 6, (empty, total)        # the second x segment holds hidden salt only: the call cannot pass by skipping nothing
    assert len(want_mid[0]) > 1000 and len(want_mid[3]) > 1000
    dense = check(ctx, labels, want_mid, colors=SKIP_COLORS, what="dense")
    sparse = check(ctx, labels, want_mid, colors=SKIP_COLORS, map_extent=map_extent, what="map %s" % (map_extent,))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(dense, sparse))
    check(ctx, labels, want_vol, colors=SKIP_COLORS, vol=vol, iso=ISO, map_extent=map_extent, cap_v=len(want_vol[0]) // 2, cap_t=len(want_vol[3]) // 3,
          what="map %s, volume, short capacities" % (map_extent,))


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(ctx):
    labels = random_labels((19, 5, 258), 21)
    vol = mesh_contents("random", (19, 5, 258), seed=22)
    want = label_indexed_np(labels, None, vol, ISO)
    a = check(ctx, labels, want, vol=vol, iso=ISO, what="first run")
    b = check(ctx, labels, want, vol=vol, iso=ISO, what="second run")
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_one_call_captured_into_a_graph_replays(ctx):
    shape = (17, 9, 131)
    labels = random_labels(shape, 13)
    vol = mesh_contents("random", shape, seed=14)
    colors = LB.color_table(3, hidden=(2,))
    cap_v, cap_t = 7 * 17 * 9 * 131, 24 * 16 * 8 * 130
    d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
    d_vol = torch.from_numpy(vol).cuda()
    d_col = torch.from_numpy(colors.view(np.int32)).cuda()
    d_scratch = torch.empty((LB.mesh_indexed_scratch_bytes(ext_of(shape)) // 8,), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros((4,), dtype=torch.int64, device="cuda")
    d_vert = torch.empty((cap_v, 3), dtype=torch.float32, device="cuda")
    d_norm = torch.empty((cap_v, 3), dtype=torch.float32, device="cuda")
    d_pair = torch.empty((cap_v, 2), dtype=torch.int32, device="cuda")
    d_idx = torch.empty((cap_t, 3), dtype=torch.int32, device="cuda")
    d_tl = torch.empty((cap_t,), dtype=torch.int32, device="cuda")
    outs = (d_vert, d_norm, d_pair, d_idx, d_tl)
    s = torch.cuda.Stream()

    def call():
        ctx.check(ctx.label_mesh_indexed_rc(d_lab.data_ptr(), ext_of(shape), None, d_col.data_ptr(), len(colors), d_vol.data_ptr(), ISO, None, None,
                                            d_scratch.data_ptr(), d_vert.data_ptr(), d_norm.data_ptr(), d_pair.data_ptr(), cap_v, d_idx.data_ptr(),
                                            d_tl.data_ptr(), cap_t, d_counts.data_ptr(), s.cuda_stream))

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
        for t in outs:
            t.view(torch.uint8).fill_(FILL)
        d_counts.fill_(-1)
        d_scratch.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        wv, wn, wp, wf, wl = label_indexed_np(labels, colors, vol, ISO)
        nv, nt = len(wv), len(wf)
        assert d_counts.cpu().tolist() == [nt, nt, nv, nv] and 0 < nv <= cap_v and 0 < nt <= cap_t
        same_u32(d_vert[:nv].cpu().numpy(), wv, "replay, seed %d: vertices" % seed)
        same_u32(d_norm[:nv].cpu().numpy(), wn, "replay, seed %d: normals" % seed)
        same_u32(d_pair[:nv].cpu().numpy().view(np.uint32), wp, "replay, seed %d: vertex labels" % seed)
        same_u32(d_idx[:nt].cpu().numpy().view(np.uint32), wf.astype(np.uint32), "replay, seed %d: indices" % seed)
        same_u32(d_tl[:nt].cpu().numpy().view(np.uint32), wl, "replay, seed %d: triangle labels" % seed)
        assert all(bool((t[n:].view(torch.uint8) == FILL).all()) for t, n in ((d_vert, nv), (d_norm, nv), (d_pair, nv), (d_idx, nt), (d_tl, nt)))
        replays.append(tuple(t.cpu().numpy().tobytes() for t in outs))
    assert replays[1] == replays[2]


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    lab = torch.full((d, h, w), 3, dtype=torch.int32, device="cuda")
    lab[1:3, 1:4, 2:9] = 1
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    col = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    # [scratch 4096 | counts 32 | vertices 2016 | normals 2048 | vertex labels 2048 | indices 2048 | triangle labels 2048]
    out = torch.full((16384,), FILL, dtype=torch.uint8, device="cuda")
    a = out.data_ptr()
    assert a % 8 == 0 and LB.mesh_indexed_scratch_bytes(e) <= 4096
    ok = dict(L=lab.data_ptr(), e=e, box=None, c=col.data_ptr(), n=4, v=vol.data_ptr(), iso=0.5, m=None, me=None, scratch=a, vert=a + 4128, norm=a + 6144,
              pair=a + 8192, cap_v=10, idx=a + 10240, tl=a + 12288, cap_t=10, counts=a + 4096)
    me = abi.Extent3D(3, 2, 1)
    bad, inf, nan = abi.VKV_E_INVALID_ARGUMENT, float("inf"), float("nan")

    def call(**change):
        k = dict(ok, **change)
        return ctx.label_mesh_indexed_rc(k["L"], k["e"], k["box"], k["c"], k["n"], k["v"], k["iso"], k["m"], k["me"], k["scratch"], k["vert"], k["norm"], k["pair"],
                                         k["cap_v"], k["idx"], k["tl"], k["cap_t"], k["counts"], st())

    # everything vkv_label_mesh rejects
    assert call(L=None) == bad and call(scratch=None) == bad and call(counts=None) == bad
    assert call(e=abi.Extent3D(w, 0, d)) == bad
    assert call(box=abi.Box(0, 0, 0, 13, 2, 2)) == bad and "box" in ctx.last_error()
    assert call(box=abi.Box(11, 4, 3, 1, 2, 1)) == bad and call(box=abi.Box(1, 1, 1, 2, 0, 2)) == bad
    for iso in (inf, -inf, nan):
        assert call(iso=iso) == bad and "iso" in ctx.last_error()
    assert call(c=None) == bad and "d_colors" in ctx.last_error()        # four entries and no table
    assert call(m=ok["v"], c=None, n=0, me=me) == bad and "d_colors" in ctx.last_error()        # a map, but no table it was built from
    assert call(m=ok["v"]) == bad and "map_extent" in ctx.last_error()
    assert call(m=ok["v"], me=abi.Extent3D(13, 2, 1)) == bad
    # and the indexed mesh's list
    assert call(cap_v=1 << 32) == bad and "32-bit" in ctx.last_error()
    assert call(vert=None, norm=None, pair=None) == bad and "d_vertices" in ctx.last_error()
    assert call(vert=None) == bad
    assert call(idx=None) == bad and "d_indices" in ctx.last_error()
    assert call(tl=None) == bad and "d_triangle_labels" in ctx.last_error()
    assert call(cap_v=0, vert=None, pair=None) == bad and "d_normals" in ctx.last_error()
    assert call(cap_v=0, vert=None, norm=None) == bad and "d_vertex_labels" in ctx.last_error()
    assert call(cap_v=0) == bad
    assert call(v=None) == bad and "d_volume" in ctx.last_error()        # normals without the volume they come from
    for name in ("L", "c", "vert", "norm", "pair", "idx", "tl"):
        assert call(**{name: ok[name] + 2}) == bad and "aligned" in ctx.last_error(), name
    assert call(norm=ok["norm"] + 1) == bad
    assert call(scratch=ok["scratch"] + 4) == bad and call(counts=ok["counts"] + 4) == bad
    assert call(e=abi.Extent3D(0x80000000, 2, 2)) == abi.VKV_E_UNSUPPORTED
    assert call(e=abi.Extent3D(2048, 2048, 1024)) == abi.VKV_E_UNSUPPORTED and "2^32" in ctx.last_error()
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # and the accepted call next to them: a non-finite iso without a volume is ignored, and so is map_extent without a map
    assert call(v=None, norm=None, iso=nan, me=me, cap_v=0, vert=None, pair=None, cap_t=0, idx=None, tl=None) == abi.VKV_OK
    torch.cuda.synchronize()
    want = label_indexed_np(lab.cpu().numpy().view(np.uint32), col.cpu().numpy().view(np.uint32))
    assert out[4096:4128].view(torch.int64).tolist() == [len(want[3]), 0, len(want[0]), 0] and len(want[0]) > 0
    assert bool((out[4128:] == FILL).all())


# ---- Volume.extract_label_mesh_indexed ----------------------------------------------------------------------------------------------------
def test_volume_extract_label_mesh_indexed_matches_the_c_call(ctx):
    vol = mesh_contents("random", (12, 13, 14), seed=61)
    v = make_volume(ctx, vol, block=2, packed=False)
    iso = 0.8
    labels = v.label_components(iso, connectivity=14, sizes=False)[0]
    h_labels = labels.cpu().numpy().view(np.uint32)
    assert h_labels.max() > 3
    want = label_indexed_np(h_labels, None, vol, iso)
    nv, nt = len(want[0]), len(want[3])
    c = run(ctx, h_labels, nv, nt, vol=vol, iso=iso, what="C call")
    assert c[0].tolist() == [nt, nt, nv, nv]

    def same(got, c_call, what, counts=None):
        vertices, faces, face_labels, normals, pairs = got
        assert vertices.dtype == torch.float32 and faces.dtype == torch.uint32 and face_labels.dtype == torch.uint32
        assert tuple(vertices.shape) == c_call[1].shape and tuple(faces.shape) == c_call[4].shape and tuple(face_labels.shape) == c_call[5].shape
        same_u32(vertices.cpu().numpy(), c_call[1], what + ": vertices")
        same_u32(faces.cpu().numpy(), c_call[4], what + ": faces")
        same_u32(face_labels.cpu().numpy(), c_call[5], what + ": face labels")
        if normals is not None:
            assert normals.dtype == torch.float32
            same_u32(normals.cpu().numpy(), c_call[2], what + ": normals")
        if pairs is not None:
            assert pairs.dtype == torch.uint32 and tuple(pairs.shape) == c_call[3].shape
            same_u32(pairs.cpu().numpy(), c_call[3], what + ": vertex labels")

    got = v.extract_label_mesh_indexed(labels, iso=iso, normals=True, vertex_labels=True)
    assert len(got) == 5 and got[3] is not None and got[4] is not None
    same(got, c, "everything")
    got = v.extract_label_mesh_indexed(labels, iso=iso)
    assert got[3] is None and got[4] is None
    same(got, c, "neither normals nor vertex labels")
    iso_vertices, iso_faces, iso_normals = v.extract_isosurface_indexed(iso, normals=True)
    same_u32(got[0].cpu().numpy(), iso_vertices.cpu().numpy(), "extract_isosurface_indexed: vertices")
    same_u32(got[1].cpu().numpy(), iso_faces.cpu().numpy(), "extract_isosurface_indexed: faces")
    tri, tri_labels, total = v.extract_label_mesh(labels, iso=iso)
    same_bits(got[0].cpu().numpy()[got[1].cpu().numpy().astype(np.int64)], tri.cpu().numpy(), "against extract_label_mesh")
    assert np.array_equal(got[2].cpu().numpy(), tri_labels.cpu().numpy())
    # midpoints, two labels hidden, with and without the visibility map
    colors = LB.color_table(int(h_labels.max()), hidden=(1, 3))
    d_colors = torch.from_numpy(colors.view(np.int32)).to(labels.device)
    want = label_indexed_np(h_labels, colors)
    nv, nt = len(want[0]), len(want[3])
    c = run(ctx, h_labels, nv, nt, colors=colors, what="C call, midpoints")
    same(v.extract_label_mesh_indexed(labels, d_colors, vertex_labels=True), c, "midpoints, two labels hidden")
    with pytest.raises(RuntimeError):
        v.extract_label_mesh_indexed(labels, d_colors, use_visibility_map=True)
    v.build_label_visibility_map(labels, d_colors)
    same(v.extract_label_mesh_indexed(labels, d_colors, vertex_labels=True, use_visibility_map=True), c, "visibility map")
    c = run(ctx, h_labels, 100, 50, colors=colors, what="C call, capacities")
    got = v.extract_label_mesh_indexed(labels, d_colors, vertex_labels=True, use_visibility_map=True, capacity=(100, 50))
    assert len(got) == 6 and got[5].cpu().tolist() == [nt, 50, nv, 100]
    same(got[:5], c, "capacity (100, 50)")
    got = v.extract_label_mesh_indexed(labels, capacity=(0, 0))
    assert tuple(got[0].shape) == (0, 3) and tuple(got[1].shape) == (0, 3) and tuple(got[2].shape) == (0,) and got[5].cpu().tolist()[1::2] == [0, 0]
    box = ((2, 3, 1), (7, 6, 9))
    sub = bordered(random_labels((7, 4, 5), 62))
    d_sub = torch.from_numpy(np.ascontiguousarray(sub).view(np.int32)).to(labels.device)
    want = label_indexed_np(sub, None, vol, iso, (2, 3, 1, 7, 6, 9))
    c = run(ctx, sub, len(want[0]), len(want[3]), vol=vol, iso=iso, box=(2, 3, 1, 7, 6, 9), what="C call, box")
    same_u32(c[1], want[0], "box: the C call's vertices")
    same(v.extract_label_mesh_indexed(d_sub, iso=iso, box=box, normals=True, vertex_labels=True), c, "box")
    empty = v.extract_label_mesh_indexed(torch.zeros_like(labels), iso=iso, normals=True, vertex_labels=True)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3), (0,), (0, 3), (0, 2)]
    with pytest.raises(ValueError):
        v.extract_label_mesh_indexed(labels, normals=True)        # normals are the volume's: they need iso
    with pytest.raises(ValueError):
        v.extract_label_mesh_indexed(labels, box=box)
    with pytest.raises(ValueError):
        v.extract_label_mesh_indexed(labels, d_colors[:0])
    with pytest.raises(ValueError):
        v.extract_label_mesh_indexed(labels, capacity=(1 << 32, 1))
