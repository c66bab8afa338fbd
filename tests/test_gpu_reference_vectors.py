"""The HIP kernels against outputs of the reference's OWN shader text (tests/golden/reference_v1.npz, written by
tests/golden/make_reference_vectors.py from the compiled shaders where a checkout of the reference was present).  Here only the committed file is
read - neither the reference nor the library built from it exists on a GPU machine - and the inputs are regenerated from their seeds and checked
against the hashes the file keeps.  No value in the file came from oracle/vkv_oracle.c, so a misreading that the oracle and the kernels share
fails here.  Maps: every byte.  Frames (36 x 30 x 26 voxels, 48 x 48 pixels, every skipping type with and without early ray termination): the three
counters of every pixel equal, colour within COLOR_TOL, depth within DEPTH_TOL - through the linear buffers and the packed image, both
schedulers, and address_tables 0 / 1 / 2."""
import numpy as np
import pytest
import torch

from tests.golden import make_reference_vectors as G
from tests.test_gpu_parity import COLOR_TOL, DEPTH_TOL, dev, gpu_render, make_gpu_volume
from vkvolume_amd import abi, volume as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    g = np.load(G.PATH)
    for key, digest in G.input_hashes().items():
        assert str(g[key]) == digest, "the regenerated input behind %s is not the one the fixture was made from" % key
    return g


def stream():
    return torch.cuda.current_stream().cuda_stream


CASES = {"": (G.volume, G.BLOCK), "small_": (G.small_volume, G.SMALL_BLOCK)}


@pytest.mark.parametrize("case", list(CASES))
def test_gradient_and_occupancy_maps(ctx, gold, case):
    """vkv_gradient_map and vkv_occupancy_map with the precomputed and the on-the-fly gradient"""
    make, block = CASES[case]
    scene = G.scene_for(make(), block)
    v, tf = make_gpu_volume(ctx, scene)
    assert np.array_equal(v.gradient.cpu().numpy(), gold[case + "gradient"])
    d_grad = torch.full(scene.vol.shape, 0xA5, dtype=torch.uint8, device="cuda")
    ctx.gradient_map(v.volume.data_ptr(), d_grad.data_ptr(), v.extent, tf, stream())
    assert np.array_equal(d_grad.cpu().numpy(), gold[case + "gradient"])
    for key, grad in (("occupancy_precomputed", v.gradient.data_ptr()), ("occupancy_on_the_fly", None)):
        expect = gold[case + key]
        d_map = torch.full(expect.shape, 77, dtype=torch.uint8, device="cuda")
        ctx.occupancy_map(v.volume.data_ptr(), grad, v.transfer_function.data_ptr(), tf, v.extent, d_map.data_ptr(), v.map_extent, stream())
        assert np.array_equal(d_map.cpu().numpy(), expect), key


def transforms(ctx, occ):
    d, h, w = occ.shape
    d_map, d_swap = dev(occ), torch.empty(occ.shape, dtype=torch.uint8, device="cuda")
    ctx.distance_map(d_map.data_ptr(), d_swap.data_ptr(), abi.Extent3D(w, h, d), stream())
    maps = [torch.full(occ.shape, 0x5A, dtype=torch.uint8, device="cuda") for _ in range(8)]
    maps[7].copy_(dev(occ))
    ctx.distance_map_anisotropic([m.data_ptr() for m in maps], d_swap.data_ptr(), abi.Extent3D(w, h, d), stream())
    return d_map.cpu().numpy(), np.stack([m.cpu().numpy() for m in maps])


@pytest.mark.parametrize("case", ["", "small_", "sparse_"])
def test_distance_transforms(ctx, gold, case):
    """vkv_distance_map and vkv_distance_map_anisotropic on the reference's occupancy maps and on a sparse map of its own"""
    occ = G.sparse_occupancy() if case == "sparse_" else gold[case + "occupancy_precomputed"]
    iso, aniso = transforms(ctx, occ)
    assert np.array_equal(iso, gold[case + "distance"])
    for k in range(8):
        assert np.array_equal(aniso[k], gold[case + "distance_aniso"][k]), "octant %d" % k


@pytest.fixture(scope="module")
def gpu_scene(ctx, gold):
    scene = G.scene_for(G.volume(), G.BLOCK)
    v, tf = make_gpu_volume(ctx, scene)
    return scene, v, tf, V.ComputeDistanceMap(ctx)


def test_compute_distance_map(ctx, gold, gpu_scene):
    """vkv_compute_distance_map: occupancy and transform in one call, every skipping type"""
    scene, v, tf, cdm = gpu_scene
    for mode, key in ((abi.SKIP_BLOCK, "occupancy_precomputed"), (abi.SKIP_DISTANCE, "distance"), (abi.SKIP_ANISOTROPIC_DISTANCE, "distance_aniso")):
        cdm.compute(v, tf, mode)
        torch.cuda.synchronize()
        expect = gold[key] if mode == abi.SKIP_ANISOTROPIC_DISTANCE else gold[key][None]
        assert len(v.distance_maps) == len(expect)
        for k in range(len(expect)):
            assert np.array_equal(v.distance_maps[k].cpu().numpy(), expect[k]), "mode %d map %d" % (mode, k)


def assert_frame(gold, key, color, counts, depth, what):
    expect = gold["counts_" + key].astype(np.uint32)
    assert expect[..., 0].sum() > 1000
    assert np.array_equal(counts, expect), "%s: counters differ in %d pixels" % (what, int((counts != expect).any(-1).sum()))
    dc, dd = float(np.abs(color - gold["color_" + key]).max()), float(np.abs(depth - gold["depth_" + key]).max())
    print("%s: colour differs by %g, depth by %g" % (what, dc, dd))
    assert dc <= COLOR_TOL, "%s: colour differs by %g" % (what, dc)
    assert dd <= DEPTH_TOL, "%s: depth differs by %g" % (what, dd)


@pytest.mark.parametrize("ert", [True, False])
@pytest.mark.parametrize("mode", G.MODES)
def test_render(ctx, gold, gpu_scene, mode, ert):
    """vkv_render; gpu_render runs the packed image and the linear buffers under both schedulers and requires the same bits of all four"""
    scene, v, tf, cdm = gpu_scene
    cdm.compute(v, tf, mode)
    color, counts, depth, _ = gpu_render(ctx, v, G.frame_params(scene, mode, ert))
    assert_frame(gold, "m%d_e%d" % (mode, ert), color, counts, depth, "mode %d ert %d" % (mode, ert))


@pytest.mark.parametrize("tables", [0, 1, 2])
@pytest.mark.parametrize("mode", G.MODES)
def test_render_address_tables(ctx, gold, gpu_scene, mode, tables):
    """the same frames with the packed image addressed by arithmetic in registers (0), two-level tables (1) and per-voxel tables (2)"""
    scene, v, tf, cdm = gpu_scene
    cdm.compute(v, tf, mode)
    size = G.IMAGE
    ctx.set_tuning(address_tables=tables)
    try:
        for ert in (True, False):
            p = G.frame_params(scene, mode, ert)
            sp = V.VolumeRenderSubpass(ctx, v, p.options, size)
            color = torch.full((size[1], size[0], 4), -1.0, dtype=torch.float32, device="cuda")
            counts = torch.full((size[1], size[0], 3), 0xFFFF, dtype=torch.int32, device="cuda")
            depth = torch.full((size[1], size[0]), -1.0, dtype=torch.float32, device="cuda")
            q = sp.bind(p)
            assert bool(q.d_packed_volume)
            sp.draw(q, color, None, counts, depth)
            torch.cuda.synchronize()
            assert_frame(gold, "m%d_e%d" % (mode, ert), color.cpu().numpy(), counts.cpu().numpy().astype(np.uint32), depth.cpu().numpy(),
                         "mode %d ert %d address_tables %d" % (mode, ert, tables))
    finally:
        ctx.set_tuning(address_tables=2)
