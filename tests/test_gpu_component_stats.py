"""GPU: vkv_component_stats and vkv_select_components_by_table bit for bit against the numpy statements of
tests/test_component_stats_cpu.py (component_stats_np, select_by_table_np): every byte of every 80-byte record, every byte of the selected
volume.  Labels come from components_np() or are built in numpy (the call takes any label array), so only the integration test depends on
the device's labelling.

The accumulate kernel is one-dimensional over the box-linear voxel index: a wave's 64 consecutive voxels are one ENTRY, a wave walks a SPAN
of 32 entries (2048 voxels) and a workgroup sixteen spans.  The extents are those of tests/test_gpu_components.py (axes of length 1, fewer
voxels than a wave, one short of, at and one past one and two entries, narrow boxes whose entries wrap many rows and slices) and 7x3x3,
131x3x2, 130x17x5 (173 entries: six spans, walked by six waves that meet in LDS) and 130x17x17 (588 entries: more than the 512 of one
workgroup of sixteen waves); what the particular shapes below reach is asserted from numpy alone in tests/test_component_stats_cpu.py.
Every buffer is a tests/helpers.py guarded() allocation, pre-filled and
compared as a whole: an unwritten byte shows as the pre-fill, a byte beyond the written records must still hold it, all guards must be intact
and the inputs unchanged, so nothing here relies on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_component_stats_cpu import (BORDER_BOX, DTYPE, SLAB_EXTENT, STATS_EXTENTS, X_NEEDLE, border_volume, clear_border_np, component_stats_np,
                                            own_labels, select_by_table_np, survivors)
from tests.test_components_cpu import components_np
from tests.test_gpu_components import CONNECTIVITIES, CONTENTS, contents
from tests.test_gpu_mesh import BOX_VOLUME, BOXES, FILL, ISO, ext_of, st
from tests.test_gpu_mesh_indexed import guard_damage
from tests.test_gpu_mip import make_volume
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu

RECORD = 80
GARBAGE = 0x7123456789abcdef        # d_counts[1] and d_counts[2]: not read


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


def shaded(vol, seed=0):
    """the same inside voxels (>= 128) with many byte values instead of two"""
    rng = np.random.default_rng(seed)
    return np.where(vol >= 128, rng.integers(128, 256, size=vol.shape), rng.integers(0, 128, size=vol.shape)).astype(np.uint8)


def stats(ctx, vol, labels, n_labels, cap, box=None, values=True, vol_offset=0, vol_fill=0x00, extra=3, what=""):
    """the whole record buffer (cap + extra records, as bytes) of ONE vkv_component_stats call on guarded buffers, pre-filled with FILL"""
    abox = None if box is None else abi.Box(*box)
    d_vol, h_vol = T.guarded(vol, vol_offset, vol_fill, "cuda")
    d_labels, h_labels = T.guarded(np.ascontiguousarray(labels).view(np.int32), 0, FILL, "cuda")
    counts = np.array([n_labels, GARBAGE, GARBAGE], np.uint64)
    d_counts, h_counts = T.guarded(counts.view(np.int64), 0, FILL, "cuda")
    d_stats, h_stats = T.guarded(((cap + extra) * RECORD,), 0, FILL, "cuda")
    ctx.component_stats(d_vol.data_ptr() if values else None, ext_of(vol), abox, d_labels.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(), cap, st())
    torch.cuda.synchronize()
    for name, h in (("d_volume", h_vol), ("d_labels", h_labels), ("d_counts", h_counts), ("d_stats", h_stats)):
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    assert np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    assert np.array_equal(d_labels.cpu().numpy().view(np.uint32), labels) and np.array_equal(d_counts.cpu().numpy().view(np.uint64), counts), what
    return d_stats.cpu().numpy()


def expected_bytes(rec, records):
    want = np.full(records * RECORD, FILL, np.uint8)
    want[:len(rec) * RECORD] = np.frombuffer(rec.tobytes(), np.uint8)
    return want


def same_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        k = int(np.flatnonzero(bad)[0]) // RECORD
        g, w = got[k * RECORD:(k + 1) * RECORD].view(DTYPE)[0], want[k * RECORD:(k + 1) * RECORD].view(DTYPE)[0]
        raise AssertionError("%s: %d bytes differ, first in record %d of %d: got %s want %s" % (what, int(bad.sum()), k, len(got) // RECORD, g, w))


def check(ctx, vol, labels, n_labels, cap=None, box=None, values=True, what="", **kw):
    """one call against the statement: the exact records [0, min(n_labels, cap)) and the pre-fill behind them"""
    cap = n_labels + 5 if cap is None else cap
    got = stats(ctx, vol, labels, n_labels, cap, box=box, values=values, what=what, **kw)
    rec = component_stats_np(vol if values else None, labels, n_labels, cap, box)
    assert len(rec) == min(n_labels, cap)
    same_records(got, expected_bytes(rec, len(got) // RECORD), what)
    return rec


# ---- extents and contents ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", STATS_EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_content_and_connectivity(ctx, extent):
    w, h, d = extent
    for k, content in enumerate(CONTENTS):
        vol = shaded(contents(content, (d, h, w), seed=900 + k), seed=k)
        for c in CONNECTIVITIES:
            labels, sizes, counts = components_np(vol, ISO, c)
            what = "%s %s, %d" % (content, extent, c)
            rec = check(ctx, vol, labels, int(counts[0]), what=what)
            assert np.array_equal(rec["voxels"], sizes), what
        check(ctx, vol, labels, int(counts[0]), values=False, what=what + ", no volume")


def test_one_component_reaches_64_bit_sums(ctx):
    w, h, d = SLAB_EXTENT
    rec = check(ctx, np.full((d, h, w), 255, np.uint8), np.ones((d, h, w), np.uint32), 1, cap=1, what="slab %s" % (SLAB_EXTENT,))
    assert rec["sum_x"][0] > 2 ** 32 and rec["sum_value2"][0] > 2 ** 32


def test_the_x_needle_reaches_the_64_bit_span_partial(ctx):
    vol = np.random.default_rng(4).integers(0, 256, size=(1, 1, X_NEEDLE), dtype=np.uint8)
    rec = check(ctx, vol, np.ones((1, 1, X_NEEDLE), np.uint32), 1, cap=1, what="x-needle")
    assert rec["sum_x"][0] == X_NEEDLE * (X_NEEDLE - 1) // 2 and rec["max_x"][0] == X_NEEDLE - 1


@pytest.mark.parametrize("shape", [(1, 5000, 1), (5000, 1, 1)], ids=["y", "z"])
def test_y_and_z_needles(ctx, shape):
    vol = np.random.default_rng(5).integers(0, 256, size=shape, dtype=np.uint8)
    i = np.arange(5000)
    check(ctx, vol, np.ones(shape, np.uint32), 1, what="needle %s, one label" % (shape,))
    check(ctx, vol, (1 + i // 700 % 3 * (i % 5 != 0)).astype(np.uint32).reshape(shape), 3, what="needle %s, three labels in runs" % (shape,))
    check(ctx, vol, own_labels(shape), 5000, what="needle %s, own labels" % (shape,))


@pytest.mark.parametrize("shape", [(2, 3, 128), (5, 17, 130)], ids=lambda s: "%dx%dx%d" % s[::-1])
def test_every_voxel_its_own_component(ctx, shape):
    """the worst cases of the reduction loop: the checkerboard under 6 (32 one-voxel labels per entry) and a label per voxel (64)"""
    vol = contents("checkerboard", shape)
    labels, sizes, counts = components_np(vol, ISO, 6)
    assert (sizes == 1).all() and counts[0] == (vol != 0).sum()
    check(ctx, vol, labels, int(counts[0]), what="checkerboard %s" % (shape,))
    vol = np.random.default_rng(9).integers(0, 256, size=shape, dtype=np.uint8)
    check(ctx, vol, own_labels(shape), vol.size, what="own labels %s" % (shape,))
    check(ctx, vol, own_labels(shape)[::-1, ::-1, ::-1].copy(), vol.size, what="own labels backwards %s" % (shape,))


# ---- boxes -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box_volume():
    w, h, d = BOX_VOLUME
    return shaded(contents("random 0.45", (d, h, w), seed=91), seed=2)


@pytest.mark.parametrize("box", sorted(BOXES), ids=lambda b: b.replace(" ", "_").replace(",", ""))
def test_a_box_is_measured_in_volume_coordinates(ctx, box_volume, box):
    b = BOXES[box]
    x0, y0, z0, w, h, d = b
    for c in (6, 26):
        labels, sizes, counts = components_np(box_volume, ISO, c, b)
        rec = check(ctx, box_volume, labels, int(counts[0]), box=b, what="box %s, %d" % (box, c))
        if len(rec):
            assert rec["min_x"].min() >= x0 and rec["max_x"].max() < x0 + w and rec["min_z"].min() >= z0 and rec["max_y"].max() < y0 + h
        check(ctx, box_volume, labels, int(counts[0]), box=b, values=False, cap=max(int(counts[0]) - 1, 0), what="box %s, %d, no volume, short" % (box, c))


# ---- capacities, empty labels, no volume -------------------------------------------------------------------------------------------------------
def test_capacities_give_exact_prefixes(ctx):
    vol = shaded(contents("random 0.2", (18, 6, 70), seed=3))
    for c in CONNECTIVITIES:
        labels, sizes, counts = components_np(vol, ISO, c)
        k = int(counts[0])
        assert k > 20
        for cap in (0, 1, k - 1, k, k + 5):
            rec = check(ctx, vol, labels, k, cap=cap, what="capacity %d of %d, %d" % (cap, k, c))
            assert len(rec) == min(cap, k)


def test_empty_labels_hold_the_identities(ctx):
    vol = shaded(contents("random 0.31", (5, 9, 67), seed=8))
    labels, sizes, counts = components_np(vol, ISO, 6)
    k = int(counts[0])
    sparse = np.where(labels % 3 == 0, 0, labels).astype(np.uint32)        # every third label loses all its voxels
    for values in (True, False):
        rec = check(ctx, vol, sparse, k + 40, values=values, what="labels with gaps, n_labels beyond the largest")
        gone = rec[2::3]
        assert len(rec) == k + 40 and not gone["voxels"].any() and (gone["min_x"] == 0xffffffff).all() and not gone["max_x"].any()
        assert (rec[k:]["min_z"] == 0xffffffff).all() and (rec["min_value"][2::3] == (0xffffffff if values else 0)).all()
    rec = check(ctx, vol, np.zeros_like(labels), 7, what="no label at all")
    assert not rec["voxels"].any()
    check(ctx, vol, labels, 0, what="n_labels 0: every voxel is above it")


def test_no_volume_leaves_the_value_fields_zero_and_the_rest_unchanged(ctx):
    vol = shaded(contents("random 0.31", (6, 7, 131), seed=15))
    labels, sizes, counts = components_np(vol, ISO, 26)
    k = int(counts[0])
    with_values = check(ctx, vol, labels, k, what="with the volume")
    without = check(ctx, vol, labels, k, values=False, what="without the volume")
    for f in DTYPE.names:
        if "value" in f:
            assert not without[f].any() and with_values[f].any()
        else:
            assert np.array_equal(without[f], with_values[f])


@pytest.mark.parametrize("extent", [(7, 3, 3), (131, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_volume_alignment_with_both_guard_fills(ctx, extent):
    """a result that consumed a guard byte as a voxel differs under one of the two fills"""
    w, h, d = extent
    vol = shaded(contents("random 0.4", (d, h, w), seed=77))
    for c in (6, 26):
        labels, sizes, counts = components_np(vol, ISO, c)
        for fill in (0x00, 0xFF):
            for offset in (0, 1, 2, 3):
                check(ctx, vol, labels, int(counts[0]), vol_offset=offset, vol_fill=fill, what="%s, %d, volume +%d fill %#x" % (extent, c, offset, fill))


# ---- integration, determinism, capture ---------------------------------------------------------------------------------------------------------
def test_voxels_equal_the_sizes_of_the_label_call(ctx):
    vol = shaded(contents("random 0.31", (19, 5, 258), seed=21))
    d_vol = torch.from_numpy(vol).cuda()
    d_scratch = torch.empty((lib.components_scratch_bytes(ext_of(vol)) // 8,), dtype=torch.int64, device="cuda")
    for c in CONNECTIVITIES:
        wl, ws, wc = components_np(vol, ISO, c)
        k = int(wc[0])
        d_labels = torch.empty(vol.shape, dtype=torch.int32, device="cuda")
        d_sizes = torch.empty((k,), dtype=torch.int32, device="cuda")
        d_counts = torch.empty((3,), dtype=torch.int64, device="cuda")
        d_stats = torch.full((k, RECORD), FILL, dtype=torch.uint8, device="cuda")
        ctx.label_components(d_vol.data_ptr(), ext_of(vol), None, ISO, c, None, None, d_scratch.data_ptr(), d_labels.data_ptr(), d_sizes.data_ptr(), k,
                             d_counts.data_ptr(), st())
        ctx.component_stats(d_vol.data_ptr(), ext_of(vol), None, d_labels.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(), k, st())        # no wait between
        torch.cuda.synchronize()
        rec = d_stats.cpu().numpy().reshape(-1).view(DTYPE)
        assert np.array_equal(rec["voxels"], d_sizes.cpu().numpy().view(np.uint32)) and int(rec["voxels"].sum()) == int(wc[2])
        same_records(d_stats.cpu().numpy().reshape(-1), expected_bytes(component_stats_np(vol, wl, k, k), k), "device labels, %d" % c)


def test_two_runs_on_the_same_buffers_give_identical_bytes(ctx):
    vol = shaded(contents("random 0.31", (19, 5, 258), seed=22))
    labels, sizes, counts = components_np(vol, ISO, 6)
    k = int(counts[0])
    d_vol, d_labels = torch.from_numpy(vol).cuda(), torch.from_numpy(labels.view(np.int32)).cuda()
    d_counts = torch.tensor([k, 0, 0], dtype=torch.int64, device="cuda")
    d_stats = torch.full((k, RECORD), FILL, dtype=torch.uint8, device="cuda")
    results = []
    for _ in range(2):        # the second run starts from the first run's records
        ctx.component_stats(d_vol.data_ptr(), ext_of(vol), None, d_labels.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(), k, st())
        torch.cuda.synchronize()
        results.append(d_stats.cpu().numpy().reshape(-1))
    assert np.array_equal(results[0], results[1])
    same_records(results[1], expected_bytes(component_stats_np(vol, labels, k, k), k), "second run")


def test_one_call_captured_into_a_graph_replays_onto_cleared_buffers(ctx):
    shape = (17, 9, 131)
    cap = 4000
    d_vol = torch.empty(shape, dtype=torch.uint8, device="cuda")
    d_labels = torch.empty(shape, dtype=torch.int32, device="cuda")
    d_counts = torch.zeros((3,), dtype=torch.int64, device="cuda")
    d_stats = torch.empty((cap, RECORD), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def load(seed):
        vol = shaded(contents("random 0.31", shape, seed=seed), seed=seed)
        labels, _, counts = components_np(vol, ISO, 26)
        d_vol.copy_(torch.from_numpy(vol))
        d_labels.copy_(torch.from_numpy(labels.view(np.int32)))
        d_counts.copy_(torch.from_numpy(counts.view(np.int64)))
        return vol, labels, int(counts[0])

    def call():
        ctx.component_stats(d_vol.data_ptr(), ext_of(d_vol), None, d_labels.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(), cap, s.cuda_stream)

    load(13)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # one direct call on the capture stream
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    torch.cuda.synchronize()
    for seed in (13, 14):  # the inputs rewritten in place (K is read on the device), the records cleared, then the graph replayed
        vol, labels, k = load(seed)
        assert 0 < k < cap
        d_stats.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        same_records(d_stats.cpu().numpy().reshape(-1), expected_bytes(component_stats_np(vol, labels, k, cap), cap), "replay, seed %d" % seed)


# ---- rejected calls ----------------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")        # [labels 2048 | counts 32 | keep 2016 | records 2048 | a volume 2048]
    a = out.data_ptr()
    assert a % 8 == 0
    labels, counts, keep, records, dst, v = a, a + 2048, a + 2080, a + 4096, a + 6144, vol.data_ptr()
    bad, unsupported = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED
    rc = lambda *args: ctx.component_stats_rc(*args, st())  # noqa: E731
    assert rc(v, e, None, None, counts, records, 10) == bad
    assert rc(v, e, None, labels, None, records, 10) == bad
    assert rc(v, e, None, labels, counts, None, 10) == bad and "d_stats" in ctx.last_error()
    assert rc(v, abi.Extent3D(w, 0, d), None, labels, counts, records, 10) == bad
    assert rc(v, e, abi.Box(1, 1, 1, 2, 0, 2), labels, counts, records, 10) == bad and "box" in ctx.last_error()
    assert rc(v, e, abi.Box(0, 0, 0, 13, 2, 2), labels, counts, records, 10) == bad and "box" in ctx.last_error()
    assert rc(v, e, abi.Box(11, 4, 3, 1, 2, 1), labels, counts, records, 10) == bad
    assert rc(v, e, None, labels + 2, counts, records, 10) == bad and "aligned" in ctx.last_error()
    assert rc(v, e, None, labels, counts + 4, records, 10) == bad
    assert rc(v, e, None, labels, counts, records + 4, 10) == bad
    assert rc(v, e, None, labels, counts, records, 1 << 32) == bad and "32-bit" in ctx.last_error()
    assert rc(v, abi.Extent3D(0x10000, 0x10000, 2), None, labels, counts, records, 10) == unsupported        # 2^33 voxels
    assert rc(v, abi.Extent3D(0x10000, 0x10000, 1), None, labels, counts, records, 10) == unsupported        # 2^32: one too many
    assert rc(None, e, None, labels, counts, None, 0) == abi.VKV_OK        # capacity 0: nothing to write, and d_stats may be null
    assert rc(v, e, None, labels, counts, records, 0) == abi.VKV_OK
    # vkv_select_components_by_table
    sel = lambda *args: ctx.select_components_by_table_rc(*args, st())  # noqa: E731
    assert sel(None, dst, e, None, labels, keep, 4, 0) == bad
    assert sel(v, None, e, None, labels, keep, 4, 0) == bad
    assert sel(v, dst, e, None, None, keep, 4, 0) == bad
    assert sel(v, dst, e, None, labels, None, 4, 0) == bad and "d_keep" in ctx.last_error()
    assert sel(v, dst, abi.Extent3D(0, h, d), None, labels, keep, 4, 0) == bad
    assert sel(v, dst, e, abi.Box(0, 0, 0, 13, 2, 2), labels, keep, 4, 0) == bad and "box" in ctx.last_error()
    assert sel(v, dst, e, abi.Box(1, 1, 1, 2, 0, 2), labels, keep, 4, 0) == bad
    assert sel(v, dst, e, None, labels, keep, 4, 256) == bad and "fill" in ctx.last_error()
    assert sel(v, dst, e, None, labels + 2, keep, 4, 0) == bad and "aligned" in ctx.last_error()
    for shift in (1, 100, w * h * d - 1):        # the two volumes overlap without being equal
        assert sel(dst, dst + shift, e, None, labels, keep, 4, 0) == bad and "overlap" in ctx.last_error()
        assert sel(dst + shift, dst, e, None, labels, keep, 4, 0) == bad
    assert sel(v, dst, abi.Extent3D(0x10000, 0x10000, 2), None, labels, keep, 4, 0) == unsupported
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # and the accepted calls next to them: every voxel in label 1, measured, then removed in place by a table that rejects it
    out[:960].view(torch.int32).fill_(1)
    out[2048:2072].view(torch.int64).copy_(torch.tensor([1, 0, 0]))
    out[2080] = 0
    assert rc(v, e, None, labels, counts, records, 10) == abi.VKV_OK
    assert sel(v, v, e, None, labels, keep + 1, 0, 7) == abi.VKV_OK        # an empty table names nothing
    torch.cuda.synchronize()
    assert bool((vol == 200).all())
    assert sel(v, v, e, None, labels, keep, 1, 7) == abi.VKV_OK
    torch.cuda.synchronize()
    rec = out[4096:4096 + RECORD].cpu().numpy().view(DTYPE)[0]
    assert rec.tolist() == (0, 0, 0, 11, 4, 3, 200, 200, 240, 240 * 11 // 2, 240 * 4 // 2, 240 * 3 // 2, 240 * 200, 240 * 40000)
    assert bool((out[4096 + RECORD:] == FILL).all()) and bool((out[2081:4096] == FILL).all()) and bool((vol == 7).all())


# ---- vkv_select_components_by_table ----------------------------------------------------------------------------------------------------------------
def select(ctx, vol, labels, keep, fill, box=None, in_place=False, what=""):
    """the whole destination volume of ONE vkv_select_components_by_table call on guarded buffers (the destination pre-filled with FILL unless in place)"""
    abox = None if box is None else abi.Box(*box)
    d_src, h_src = T.guarded(vol, 1, FILL, "cuda")
    d_dst, h_dst = (d_src, h_src) if in_place else T.guarded(vol.shape, 3, FILL, "cuda")
    d_labels, h_labels = T.guarded(labels.view(np.int32), 0, FILL, "cuda")
    table = np.asarray(keep).astype(np.uint8)
    d_keep, h_keep = T.guarded(table if len(table) else np.zeros(1, np.uint8), 3, 0x00, "cuda")        # zero guards: a read past the table would remove
    ctx.select_components_by_table(d_src.data_ptr(), d_dst.data_ptr(), ext_of(vol), abox, d_labels.data_ptr(), d_keep.data_ptr() if len(table) else None,
                                   len(table), fill, st())
    torch.cuda.synchronize()
    for name, h in (("d_src", h_src), ("d_dst", h_dst), ("d_labels", h_labels), ("d_keep", h_keep)):
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed" % (what, name, bad[:8])
    if not in_place:
        assert np.array_equal(d_src.cpu().numpy(), vol), "%s: the source changed" % what
    assert np.array_equal(d_labels.cpu().numpy().view(np.uint32), labels)
    return d_dst.cpu().numpy()


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d elements differ, first at %s: got %s want %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(),
                                                                                 want[bad][:4].tolist())


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_select_by_table_against_the_statement(ctx, connectivity):
    vol = shaded(contents("random 0.2", (9, 7, 131), seed=5), seed=1)
    labels, sizes, counts = components_np(vol, ISO, connectivity)
    k = int(counts[0])
    assert k > 20
    rng = np.random.default_rng(connectivity)
    fresh = np.full(vol.shape, FILL, np.uint8)
    tables = {"random": rng.random(k) < 0.5, "bytes": rng.integers(0, 256, k).astype(np.uint8) * (rng.random(k) < 0.6), "none": np.zeros(k, bool),
              "all": np.ones(k, bool), "shorter than K": rng.random(k // 2) < 0.3, "one entry": np.zeros(1, bool), "empty": np.zeros(0, bool),
              "longer than K": np.zeros(k + 9, bool)}
    for name, keep in tables.items():
        for fill in (0, 9):
            want = select_by_table_np(vol, labels, keep, fill)
            what = "table %s, fill %d, %d" % (name, fill, connectivity)
            same(select(ctx, vol, labels, keep, fill, what=what), want, what)
            same(select(ctx, vol, labels, keep, fill, in_place=True, what=what + ", in place"), want, what + ", in place")
    assert (select_by_table_np(vol, labels, tables["shorter than K"], 0) != select_by_table_np(vol, labels, tables["none"], 0)).any()
    assert np.array_equal(select_by_table_np(vol, labels, tables["empty"], 0), vol)
    # a box: its own labels; the bytes outside it untouched
    box = (40, 1, 2, 70, 5, 6)
    bl, bs, bc = components_np(vol, ISO, connectivity, box)
    keep = rng.random(int(bc[0])) < 0.5
    same(select(ctx, vol, bl, keep, 3, box=box, what="box"), select_by_table_np(vol, bl, keep, 3, box=box, dst=fresh), "box")
    same(select(ctx, vol, bl, keep, 3, box=box, in_place=True, what="box, in place"), select_by_table_np(vol, bl, keep, 3, box=box), "box, in place")


# ---- Volume ----------------------------------------------------------------------------------------------------------------------------------
def test_volume_component_stats_and_select_components(ctx):
    vol = shaded(contents("random 0.2", (10, 12, 70), seed=31), seed=3)
    v = make_volume(ctx, vol, block=2, packed=False)
    for box in (None, ((5, 2, 1), (40, 9, 8))):
        b = None if box is None else box[0] + box[1]
        labels, sizes, counts = v.label_components(ISO, connectivity=26, box=box)
        wl, ws, wc = components_np(vol, ISO, 26, b)
        k = int(wc[0])
        s = v.component_stats(labels, counts, box=box)
        rec = component_stats_np(vol, wl, k, k, b)
        assert len(s) == k and s.numpy().dtype == DTYPE and s.numpy().tobytes() == rec.tobytes()
        n = rec["voxels"].astype(np.float64)
        assert np.array_equal(s.voxels.cpu().numpy(), rec["voxels"].astype(np.int64)) and np.array_equal(s.voxels.cpu().numpy(), sizes.cpu().numpy())
        assert np.array_equal(s.bbox_min.cpu().numpy(), np.stack([rec["min_x"], rec["min_y"], rec["min_z"]], axis=1).astype(np.int64))
        assert np.array_equal(s.bbox_max.cpu().numpy(), np.stack([rec["max_x"], rec["max_y"], rec["max_z"]], axis=1).astype(np.int64))
        assert np.array_equal(s.min_value.cpu().numpy(), rec["min_value"]) and np.array_equal(s.max_value.cpu().numpy(), rec["max_value"])
        centroid = np.stack([rec["sum_x"], rec["sum_y"], rec["sum_z"]], axis=1).astype(np.float64) / n[:, None]
        mean = rec["sum_value"].astype(np.float64) / n
        variance = rec["sum_value2"].astype(np.float64) / n - mean * mean
        # float64 quotients of the same integers: IEEE division and one rounding per operation on both sides, so a few ulps at the most
        assert s.centroid.dtype == torch.float64 and tuple(s.centroid.shape) == (k, 3)
        np.testing.assert_allclose(s.centroid.cpu().numpy(), centroid, rtol=1e-14, atol=0)
        np.testing.assert_allclose(s.mean.cpu().numpy(), mean, rtol=1e-14, atol=0)
        np.testing.assert_allclose(s.variance.cpu().numpy(), variance, rtol=0, atol=1e-14 * 255.0 ** 2)
        geometry = v.component_stats(labels, counts, box=box, values=False, capacity=k + 4)
        assert len(geometry) == k + 4 and geometry.numpy()[:k].tobytes() == component_stats_np(None, wl, k, k, b).tobytes()
        short = v.component_stats(labels, counts, box=box, capacity=3)
        assert short.numpy().tobytes() == rec[:3].tobytes()
        # a rule from the records, applied on the device: the bright and not too small
        keep = (s.mean > 190.0) & (s.voxels >= 2)
        want = select_by_table_np(vol, wl, (mean > 190.0) & (rec["voxels"] >= 2), 5, box=b)
        out = v.select_components(labels, keep, fill=5, box=box)
        assert out.data_ptr() != v.volume.data_ptr() and (want != vol).any()
        same(out.cpu().numpy(), want, "Volume.select_components, box %s" % (box,))
        target = torch.full_like(v.volume, FILL)
        assert v.select_components(labels, keep.to(torch.uint8), fill=5, out=target, box=box) is target
        same(target.cpu().numpy(), select_by_table_np(vol, wl, (mean > 190.0) & (rec["voxels"] >= 2), 5, box=b, dst=np.full(vol.shape, FILL, np.uint8)), "out=")
    same(v.volume.cpu().numpy(), vol, "the volume itself")
    with pytest.raises(ValueError):
        v.select_components(labels, keep, fill=256, box=box)
    with pytest.raises(ValueError):
        v.select_components(labels, keep.to(torch.int32), box=box)
    with pytest.raises(ValueError):
        v.component_stats(labels, counts)        # the box's labels against the whole volume


def test_volume_clear_border_on_the_hand_made_volume(ctx):
    vol = border_volume()
    v = make_volume(ctx, vol, block=2, packed=False)
    for box, kept in ((None, {"interior", "box face only", "cut by the box"}), (BORDER_BOX, {"interior"})):
        for c in (6, 26):
            out = v.clear_border(ISO, connectivity=c, fill=3, box=None if box is None else (box[:3], box[3:]))
            same(out.cpu().numpy(), clear_border_np(vol, ISO, c, 3, box), "clear_border, box %s, %d" % (box, c))
        x0, y0, z0, w, h, d = (0, 0, 0) + vol.shape[::-1] if box is None else box
        assert survivors(out.cpu().numpy()[z0:z0 + d, y0:y0 + h, x0:x0 + w]) == kept
    same(v.volume.cpu().numpy(), vol, "the volume itself")
    # in place, with a built max map: the map afterwards is the map of the new volume
    for box in (BORDER_BOX, None):
        out = v.clear_border(ISO, fill=0, out=v.volume, box=None if box is None else (box[:3], box[3:]))
        assert out is v.volume
        vol = clear_border_np(vol, ISO, 6, 0, box)
        same(v.volume.cpu().numpy(), vol, "clear_border in place, box %s" % (box,))
        kept_map = v.max_map.clone()
        fresh = make_volume(ctx, vol, block=2, packed=False)
        same(kept_map.cpu().numpy(), fresh.max_map.cpu().numpy(), "the max map after clear_border in place, box %s" % (box,))
    nothing = make_volume(ctx, np.full((4, 5, 6), 10, np.uint8), block=2, packed=False)
    same(nothing.clear_border(ISO).cpu().numpy(), np.full((4, 5, 6), 10, np.uint8), "no component at all")
