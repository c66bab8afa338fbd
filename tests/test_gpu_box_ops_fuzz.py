"""GPU: the seeded fuzz of the volume-processing family: every box-of-voxels operation on the drawn cases of
tests/box_ops_fuzz.py, which crosses what the operations' own files walk one axis at a time: widths around the narrow-row kernels, a wave and
the x segments, boxes of every kind at every x0 mod 4, contents with bytes at the threshold, isos at a byte's float and its neighbours,
every connectivity, target, limit, weight triple, bound and table, short capacities, maps of any geometry, and every pointer at a drawn
multiple of its alignment inside a guarded allocation with a drawn guard byte and pre-fill.

This module only executes the recipe.  Per case: the volume and the other inputs come from the recipe, the expected outputs from the numpy
statements (through the references of tests/test_far_boxes_cpu.py), the call is the one tests/test_gpu_far_boxes.py makes, with the drawn
parameters; then every guard is intact, the inputs and the volume are unchanged, and every output buffer as a whole equals the reference to
the bit, with the pre-fill behind what the call is to write.  Then THE SAME CALL RUNS AGAIN on the same scratch block, as the first run left
it, with the outputs pre-filled anew, and must give the same bits: a kernel that leans on what a fresh allocation held shows here.
Everything is judged by value inside memory the test owns.  VKV_TEST_FUZZ_SEEDS sets the seeds per operation (12; profiles/box_ops_fuzz.txt
has a soak)."""
import os

import numpy as np
import pytest
import torch

from tests import box_ops_fuzz as Z
from tests import test_gpu_far_boxes as G
from tests.test_distance_cpu import TO_INSIDE, TO_OUTSIDE
from vkvolume_amd import abi, labels as LB, lib, mesh as M

pytestmark = pytest.mark.gpu
SEEDS = int(os.environ.get("VKV_TEST_FUZZ_SEEDS", str(Z.DEFAULT_SEEDS)))

st = G.st


# ---- the calls the far-box table lacks ---------------------------------------------------------------------------------------------------------
def run_label_mesh_indexed(ctx, S, want, B, what, iso=G.ISO, table=False, use_map=False, **_):
    cap_t, cap_v = want["_cap0"], want["_cap1"]
    nbytes = LB.mesh_indexed_scratch_bytes(S.e, S.abox)
    assert nbytes >= 16 and nbytes % 8 == 0, (what, nbytes)
    d_labels, d_colors, entries, d_map, map_extent = G.label_table(ctx, S, B, table, use_map)
    d_scratch, d_counts = B.scratch(nbytes), B.out("d_counts", (4,), np.int64)
    d_vert, d_norm, d_vl = B.out("d_vertices", (cap_v, 3), np.float32), B.out("d_normals", (cap_v, 3), np.float32), B.out("d_vertex_labels", (cap_v, 2), np.int32)
    d_idx, d_tl = B.out("d_indices", (cap_t, 3), np.int32), B.out("d_triangle_labels", (cap_t,), np.int32)
    ctx.check(ctx.label_mesh_indexed_rc(d_labels.data_ptr(), S.e, S.abox, d_colors, entries, S.d_vol.data_ptr(), iso, d_map, map_extent, d_scratch.data_ptr(),
                                        d_vert.data_ptr(), d_norm.data_ptr() if cap_v else None, d_vl.data_ptr() if cap_v else None, cap_v, d_idx.data_ptr(),
                                        d_tl.data_ptr(), cap_t, d_counts.data_ptr(), st()))
    return {"vertices": d_vert, "normals": d_norm, "vertex_labels": d_vl, "indices": d_idx, "triangle_labels": d_tl, "counts": d_counts}


def run_chain_mesh(ctx, S, want, B, what, iso=G.ISO, connectivity=6, passes=4, **_):
    """label, extract into short buffers, adjacency, smooth, normals over all faces and of one label: no count is read on the host in between"""
    cap_t, cap_v = want["_cap0"], want["_cap1"]
    d_scratch, d_ccounts = B.scratch(lib.components_scratch_bytes(S.e, S.abox)), B.out("d_component_counts", (3,), np.int64)
    d_labels = B.out("d_labels", S.shape, np.int32)
    ctx.label_components(S.d_vol.data_ptr(), S.e, S.abox, iso, connectivity, None, None, d_scratch.data_ptr(), d_labels.data_ptr(), None, 0, d_ccounts.data_ptr(), st())
    d_scratch2, d_counts = B.scratch(LB.mesh_indexed_scratch_bytes(S.e, S.abox), "d_scratch_mesh"), B.out("d_counts", (4,), np.int64)
    d_vert, d_idx, d_tl = B.out("d_vertices", (cap_v, 3), np.float32), B.out("d_indices", (cap_t, 3), np.int32), B.out("d_triangle_labels", (cap_t,), np.int32)
    ctx.check(ctx.label_mesh_indexed_rc(d_labels.data_ptr(), S.e, S.abox, None, 0, S.d_vol.data_ptr(), iso, None, None, d_scratch2.data_ptr(), d_vert.data_ptr(), None,
                                        None, cap_v, d_idx.data_ptr(), d_tl.data_ptr(), cap_t, d_counts.data_ptr(), st()))
    nbytes = M.adjacency_scratch_bytes(cap_v, cap_t)
    assert nbytes == lib.load().vkv_mesh_adjacency_scratch_bytes(cap_v, cap_t) and nbytes % 8 == 0 and nbytes >= 32
    d_adj, d_swap, d_pinned = B.scratch(nbytes, "d_scratch_adjacency"), B.out("d_scratch_swap", (cap_v, 3), np.float32), B.inp("d_pinned", want["_pinned"])
    d_norm, d_norm_l = B.out("d_normals", (cap_v, 3), np.float32), B.out("d_normals_of_label", (cap_v, 3), np.float32)
    ctx.check(ctx.mesh_adjacency_rc(d_idx.data_ptr(), cap_t, cap_v, d_counts.data_ptr(), d_adj.data_ptr(), st()))
    ctx.check(ctx.mesh_smooth_rc(d_vert.data_ptr(), d_swap.data_ptr(), cap_v, d_counts.data_ptr(), d_adj.data_ptr(), d_pinned.data_ptr(), Z.taubin_factors(passes), st()))
    ctx.check(ctx.mesh_vertex_normals_rc(d_vert.data_ptr(), d_idx.data_ptr(), None, 0, cap_v, cap_t, d_counts.data_ptr(), d_adj.data_ptr(), d_norm.data_ptr(), st()))
    ctx.check(ctx.mesh_vertex_normals_rc(d_vert.data_ptr(), d_idx.data_ptr(), d_tl.data_ptr(), want["_label"], cap_v, cap_t, d_counts.data_ptr(), d_adj.data_ptr(),
                                         d_norm_l.data_ptr(), st()))
    torch.cuda.synchronize()
    return {"labels": d_labels, "component_counts": d_ccounts.cpu().numpy()[[0, 2]], "vertices": d_vert, "indices": d_idx, "triangle_labels": d_tl,
            "counts": d_counts, "normals": d_norm, "normals_of_label": d_norm_l}


def run_chain_split(ctx, S, want, B, what, iso=G.ISO, connectivity=6, r2=4, erode_fill=0, **_):
    """Volume.split_bodies call by call: the eroded volume is a second volume-shaped buffer, of which only the box is ever read"""
    w, h, d = S.extent
    d_scratch, d_dist = G.distance_scratch(S, B, what), B.out("d_dist2", S.shape, np.int32)
    ctx.distance_transform(S.d_vol.data_ptr(), S.e, S.abox, iso, TO_OUTSIDE, r2 + 1, d_scratch.data_ptr(), d_dist.data_ptr(), st())
    d_eroded = B.out("d_dst", (d, h, w))
    ctx.select_by_distance(S.d_vol.data_ptr(), d_eroded.data_ptr(), S.e, S.abox, d_dist.data_ptr(), 1, r2, erode_fill, st())
    d_scratch2, d_counts = B.scratch(lib.components_scratch_bytes(S.e, S.abox), "d_scratch_components"), B.out("d_counts", (3,), np.int64)
    d_core, d_near, d_out = B.out("d_labels", S.shape, np.int32), B.out("d_nearest", S.shape, np.int32), B.out("d_out", S.shape, np.int32)
    ctx.label_components(d_eroded.data_ptr(), S.e, S.abox, iso, connectivity, None, None, d_scratch2.data_ptr(), d_core.data_ptr(), None, 0, d_counts.data_ptr(), st())
    ctx.check(ctx.nearest_target_rc(d_eroded.data_ptr(), S.e, S.abox, iso, TO_INSIDE, (1, 1, 1), None, d_scratch.data_ptr(), d_near.data_ptr(), None, st()))
    ctx.check(ctx.propagate_labels_rc(d_near.data_ptr(), d_core.data_ptr(), d_out.data_ptr(), S.e, S.abox, S.d_vol.data_ptr(), iso, st()))
    torch.cuda.synchronize()
    eroded = S.region(d_eroded).cpu().numpy()
    S.region(d_eroded).fill_(B.prefill)
    assert G.count_not(d_eroded, B.prefill) == 0, "%s: the eroded volume changed outside the box" % what
    return {"dist2": d_dist, "eroded": eroded, "core": d_core, "counts": d_counts.cpu().numpy()[[0, 2]], "nearest": d_near, "out": d_out}


# operation of the recipe: the call of tests/test_gpu_far_boxes.py (connectivity, map and in place are drawn parameters here)
CALLS = {
    "max_map_box": G.run_max_map_box, "max_map_whole": G.run_max_map_whole, "cell_summary": G.run_cell_summary, "histogram": G.run_histogram,
    "filter_binomial": G.run_filter(abi.FILTER_BINOMIAL3), "filter_median": G.run_filter(abi.FILTER_MEDIAN3), "mesh": G.run_mesh(False),
    "mesh_indexed": G.run_mesh_indexed(False), "components": G.run_components(6, False), "select_components": G.run_select_components(False),
    "component_stats": G.run_component_stats, "select_by_table": G.run_select_by_table, "distance": G.run_distance,
    "select_by_distance": G.run_select_by_distance, "distance_weighted": G.run_distance_weighted, "nearest": G.run_nearest,
    "propagate": G.run_propagate(False), "propagate_masked": G.run_propagate(True), "geodesic": G.run_geodesic,
    "visibility_map": G.run_visibility_map, "label_mesh": G.run_label_mesh, "label_mesh_indexed": run_label_mesh_indexed, "chain_mesh": run_chain_mesh,
    "chain_split": run_chain_split,
}
assert set(CALLS) == set(Z.OPS)


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("seed", range(SEEDS))
@pytest.mark.parametrize("op", sorted(Z.OPS))
def test_box_op(ctx, op, seed):
    case = Z.draw(op, seed)
    vol = Z.volume(case)
    aux = Z.inputs(case, vol)
    want = Z.reference(case, vol, aux)
    B = G.Buffers(prefill=case["prefill"], guard=case["guard"], offsets=lambda name: Z.offset_of(case, name))
    S = G.SmallScene(vol, case["box"], aux, case["params"]["me"] or (1, 1, 1), B)
    for run in ("first", "second"):
        what = "%s run of %s" % (run, case)
        if op == "max_map_whole":
            S.whole_map = None
        got = CALLS[op](ctx, S, want, B, what, **case["params"])
        torch.cuda.synchronize()
        B.check(what)
        G.compare(got, want, what, fill=case["prefill"])
        S.check_volume(what)
        if S.whole_map is not None:
            bad = G.guard_damage(S.whole_map[1])
            assert not bad, "%s: the whole volume's max map: guard bytes %s changed" % (what, bad[:8])
        B.again()
