"""GPU: vkv_label_components where workgroups merge across generations: 251 x 127 x 131 = 4 175 887 voxels, 16 313
workgroups, about eight times what an MI355X holds resident at once (at most 2048 workgroups of four waves: derived, not measured), so
trees built by workgroups that have finished are hooked, compressed and re-rooted by workgroups that start later, on other XCDs.  The
shape, the contents, the scipy.ndimage.label references and the arithmetic are those of tests/test_components_scale_cpu.py, which asserts
every figure of them without a GPU; run, check and same are those of tests/test_gpu_components.py: guarded buffers, every output pre-filled,
labels, sizes and counts compared whole, all guards intact and the volume unchanged.  Nothing is sampled; a mismatch names the first
differing voxels with their got and want labels.  One test per (content, connectivity), so that --durations shows each; no time is asserted."""
import numpy as np
import pytest
import torch

from tests.test_components_scale_cpu import (AT_LEAST_1000_UNDER_14, BOX, CONNECTIVITIES, CONTENTS, ISO, RANDOM_TABLE, SCALE, SHAPE, box_volume, volume_of,
                                             want_of)
from tests.test_gpu_components import check, run, same
from tests.test_gpu_mesh import FILL, ext_of, st
from vkvolume_amd import lib, volume as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


# ---- 1. every content under every neighbourhood -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("content", CONTENTS, ids=lambda c: c.replace(" ", "_"))
def test_every_content_and_connectivity(ctx, content, connectivity):
    check(ctx, volume_of(content, connectivity).copy(), ISO, connectivity, want_of(content, connectivity), what="%s %s, %d" % (content, SCALE, connectivity))


# ---- 2. the same voxels as a box of a larger volume ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_a_box_is_labelled_as_the_cropped_array(ctx, connectivity):
    want = want_of("random", connectivity)        # scipy on the crop
    labels, _, _ = check(ctx, box_volume(connectivity).copy(), ISO, connectivity, want, box=BOX, what="random as the box %s, %d" % (BOX, connectivity))
    assert labels.shape == SHAPE


# ---- 3. and 4. capacities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", ["half", "one"])
def test_a_capacity_below_the_count_gives_the_exact_prefix(ctx, capacity):
    """k_cc_relabel's L <= known filter with most of the atomic additions suppressed: [K, capacity, inside], exactly the first `capacity` sizes,
    the pre-fill behind them (check() compares the whole sizes buffer)"""
    want = want_of("random", 6)
    k = RANDOM_TABLE[6][0]
    cap = k // 2 if capacity == "half" else 1
    _, sizes, counts = check(ctx, volume_of("random", 6).copy(), ISO, 6, want, cap=cap, what="random %s, 6, capacity %d of %d" % (SCALE, cap, k))
    assert counts.tolist() == [k, cap, int(want[2][2])] and len(sizes) == cap and np.array_equal(sizes, want[1][:cap])


def test_a_counting_call_without_sizes_gives_the_same_labels(ctx):
    want = want_of("random", 6)
    labels, sizes, counts = run(ctx, volume_of("random", 6).copy(), ISO, 6, 0, null_sizes=True, what="counting call")
    assert counts.tolist() == [RANDOM_TABLE[6][0], 0, int(want[2][2])] and (sizes.view(np.uint8) == FILL).all()
    same(labels, want[0], "counting call: labels")


# ---- 5. dirty buffers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_runs_on_buffers_dirty_from_another_content_give_the_reference_bytes(ctx, connectivity):
    """the labels (the union-find's parent array), the sizes and the scratch hold the state of a run on a DIFFERENT content of the same shape
    (the comb along z: one component through every voxel's column) when the second run starts, and the second run's when the third does"""
    first, vol = volume_of("comb z", connectivity), volume_of("random", connectivity)
    wl, ws, wc = want_of("random", connectivity)
    k = int(wc[0])
    d_vol = torch.from_numpy(first.copy()).cuda()
    d_scratch = torch.full((lib.components_scratch_bytes(ext_of(vol)) // 8,), -1, dtype=torch.int64, device="cuda")
    d_labels = torch.full(vol.shape, -1, dtype=torch.int32, device="cuda")
    d_sizes = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    d_counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    results = []
    for r in range(3):
        if r == 1:
            d_vol.copy_(torch.from_numpy(vol.copy()))
        ctx.label_components(d_vol.data_ptr(), ext_of(vol), None, ISO, connectivity, None, None, d_scratch.data_ptr(), d_labels.data_ptr(), d_sizes.data_ptr(), k,
                             d_counts.data_ptr(), st())
        torch.cuda.synchronize()
        results.append((d_labels.cpu().numpy().view(np.uint32), d_sizes.cpu().numpy().view(np.uint32), d_counts.cpu().numpy().view(np.uint64)))
    assert results[0][2].tolist() == [1, 1, int((first >= 128).sum())] and results[0][1][0] == int((first >= 128).sum())        # the first run was the comb
    same(results[0][0], (first >= 128).astype(np.uint32), "first run (comb z), %d: labels" % connectivity)
    same(results[1][0], wl, "second run, %d: labels" % connectivity)
    same(results[1][1], ws, "second run, %d: sizes" % connectivity)
    assert results[1][2].tolist() == wc.tolist()
    for a, b, name in zip(results[1], results[2], ("labels", "sizes", "counts")):
        same(b, a, "third run against the second, %d: %s" % (connectivity, name))


# ---- 6. Volume.remove_islands -------------------------------------------------------------------------------------------------------------
def test_volume_remove_islands_at_scale(ctx):
    """keep_largest in place and min_voxels = 1000 into a copy, on the p = 0.18 case under 14, against np.where(keep[labels], vol, 0) from
    scipy's labels and sizes"""
    vol = volume_of("random", 14)
    wl, ws, wc = want_of("random", 14)
    assert int(ws.max()) == RANDOM_TABLE[14][1] and int((ws == ws.max()).sum()) == 1

    def kept(min_voxels):
        keep = np.concatenate(([True], ws >= min_voxels))        # label 0: outside voxels keep their byte
        return np.where(keep[wl], vol, 0).astype(np.uint8)

    v = V.Volume(ctx)
    v.load_from_array(vol.copy())
    out = v.remove_islands(ISO, min_voxels=1000, connectivity=14)
    torch.cuda.synchronize()
    assert out.data_ptr() != v.volume.data_ptr()
    want = kept(1000)
    assert int((ws >= 1000).sum()) == AT_LEAST_1000_UNDER_14 and int((want >= 128).sum()) == int(ws[ws >= 1000].sum(dtype=np.uint64))
    same(out.cpu().numpy(), want, "remove_islands(min_voxels=1000), 14")
    same(v.volume.cpu().numpy(), vol, "remove_islands(min_voxels=1000), 14: the volume itself")
    assert v.remove_islands(ISO, keep_largest=True, connectivity=14, out=v.volume) is v.volume
    torch.cuda.synchronize()
    want = kept(int(ws.max()))
    assert int((want >= 128).sum()) == RANDOM_TABLE[14][1]
    same(v.volume.cpu().numpy(), want, "remove_islands(keep_largest) in place, 14")
