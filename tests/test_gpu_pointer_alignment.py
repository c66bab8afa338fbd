"""GPU: the precompute and I/O kernels at every pointer alignment their launchers distinguish, inside guarded allocations.

Every launcher picks a kernel variant from its argument POINTERS as well as from the extent.  Each test below hands over buffers made by
tests/helpers.py guarded(): the payload lies `offset` bytes past a 256-byte boundary of ONE allocation, with 256 guard bytes (and the
offset) before it and 256 after.  Every case runs with the guard fill 0x00 and 0xFF - an occupied and an empty cell, black and the brightest
voxel: an input must give the reference of the payload alone under both fills (a kernel that consumes a guard byte disagrees under one of
them); an output is pre-filled as a whole and must equal the reference everywhere (an unwritten byte shows) with every guard byte intact (a
stray store lands in memory the test owns and shows by value; nothing here relies on, or can cause, a fault).

The references are not the code under test: oracle.vkv_oracle (gradient map, occupancy map, occupied-voxel count, both transforms, the
loader, the frames), the brute-force Chebyshev statements of tests/helpers.py for small maps, numpy for the tile de-interleave; where the
issue is one template against its sibling (the packed image, the region update) the result on aligned copies, pinned to the oracle by a frame.

The case on each side of every predicate where the pointer ALONE decides (the width allows the vector variant):

  launch_gradient_map, ALIGNED = width % 4 == 0 && d_vol % 4 == 0
      test_gradient_map: widths 4, 8, 64, 68, 132 with the volume at +0 (ALIGNED) and at +1, +2, +3 (not)
  launch_pack_volume, ALIGNED = width % 4 == 0 && (d_vol | d_grad) % 4 == 0
      test_pack_volume: widths 64, 68 with (volume, gradient) at (+0, +0) (ALIGNED), (+0, +1) and (+2, +0) (one pointer each) and mixed
  occupancy map and count, DWORDS = 2 with width % 4 == 0 && (d_vol | d_grad) % 4 == 0
      test_occupancy_map_and_count: widths 64, 68, 1028 with (volume, gradient) at (+0, +0) and (+4, +8) (aligned), (+0, +1), (+2, +0), (+1, +3)
  distance x pass, VEC = width % 4 == 0 && (src | dst | dst2) % 4 == 0
      test_distance_map / test_distance_map_anisotropic: widths 260, 512, 1024 (and every other width here) with all maps at multiples of 4
      (VEC) against one map at +1 or +2 (not); anisotropic: the x pass reads map 7 and writes maps 3 and 7, so the plans where only map 7
      (+1) or only map 3 (+2) is off decide it, the plan where only map 5 is off leaves it VEC
  distance y / z passes, vec = width % XT == 0 && (every src, dst, dst2) % XT == 0
      the same tests: (32, 130, 5) XT 16, (24, 300, 2) and (16, 600, 2) XT 8, (8, 400, 3) XT 4, with (map, swap) at (+0, +0) (vec), (+1, +0) and
      (+0, +2) (off by less than 4), (+4, +0), (+0, +8), (+8, +4) (multiples of 4 that XT 16, or XT 8, does not divide)
  k_fill_empty / k_occupancy_of_distance, byte head to the next 16-byte boundary
      test_map_fills_through_transfer_function_updates[update-*] (vkv_update_transfer_function; the from_summary cases write every cell from
      k_occupancy_from_summary and never launch the fill): 18 and 60 cells at +1 (head 15), +7, +8, +15 (head 1), +0 (no head);
      test_update_volume_region (k_occupancy_of_distance on every octant map at its own offset)
  k_convert_volume, vector path = raw % 16 == 0 && out % kPer == 0
      test_convert_volume: raw at +0 with out at +0 (vector) against out at +1, +7 (and +8 for 8-bit voxels), and out at +0 with raw at +1 .. +15
  launch_scatter_tiles_frames, four pixels per thread = ... && (image | src) % 16 == 0
      test_scatter_tiles: 80 x 48, 16 x 16 tiles, (image, gathered) at (+0, +0) (four pixels) against (+4, +0), (+0, +8), (+12, +12), ...
  integrator, fill_rgba8_rows when out_rgba8 % 16 == 0 && image_width % 4 == 0
      test_integrator_rgba8_target: width 208 with the target at +0 (row fill) and at +4 (not); width 210 never

These tests judge by value.  On gfx950 a misaligned global dword or 16-byte access still gives the right bytes, so a launcher predicate that
wrongly picked a vector variant for a misaligned pointer (an OR that missed octant map 5, say) would pass here: the cases show that the
results are right and that nothing outside the buffers is touched at every alignment, not which variant ran.
"""
import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_gpu_parity import dev, make_gpu_volume, sparse_occupancy
from tests.test_gpu_volume_region import SOURCES, State, expected_volume, make_source, mismatches
from vkvolume_amd import abi, lib, multigpu, volume as V

pytestmark = pytest.mark.gpu
FILLS = (0x00, 0xFF)


def st():
    return torch.cuda.current_stream().cuda_stream


def G(array_or_shape, offset, fill, dtype=np.uint8):
    return T.guarded(array_or_shape, offset, fill, "cuda", dtype)


def intact(what, **handles):
    for name, h in handles.items():
        bad = h.check()
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d of the allocation)" % (what, name, bad[:8], h.start, h.stop - 1)


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %d bytes differ, first at %s" % (what, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


# ---- gradient map --------------------------------------------------------------------------------------------------------------------
GRADIENT_OFFSETS = [(0, 0), (1, 1), (2, 3), (3, 0), (0, 3)]  # (d_volume, d_gradient): every volume offset, every output offset 0, 1, 3


def gradient_case(ctx, shape, use_gradient, seed):
    vol = T.random_volume(shape, seed=seed)
    opt = abi.VolumeOptions(**T.APP_TF) if use_gradient else abi.VolumeOptions(intensity_min=0.1, gradient_min=0.0, gradient_max=0.0)
    tf = lib.transfer_function_uniform(opt)
    assert bool(tf.use_gradient) == use_gradient
    want = O.gradient_map(vol, tf)
    for fill in FILLS:
        for vo, go in GRADIENT_OFFSETS:
            what = "shape %s volume +%d gradient +%d fill %#x" % (shape, vo, go, fill)
            d_vol, hv = G(vol, vo, fill)
            d_grad, hg = G(vol.shape, go, fill)
            ctx.gradient_map(d_vol.data_ptr(), d_grad.data_ptr(), abi.Extent3D(*shape), tf, st())
            same(d_grad, want, what)
            intact(what, volume=hv, gradient=hg)


@pytest.mark.parametrize("use_gradient", [True, False])
@pytest.mark.parametrize("width", [4, 8, 64, 68, 132, 5, 67])
def test_gradient_map(ctx, width, use_gradient):
    """k_gradient_map_tiled<ALIGNED> (use_gradient) and k_gradient_map: widths where the volume pointer alone decides ALIGNED, and 5 and 67, where
    rows start at every alignment anyway and the last dword of a row is partial."""
    gradient_case(ctx, (width, 9, 6), use_gradient, 11)


def test_gradient_map_marching_workgroups(ctx):
    """Depth 33 under gradient_segment = 3: workgroups that march over several tiles in z with the next tile prefetched, interior tiles in x."""
    ctx.set_tuning(gradient_segment=3)
    try:
        gradient_case(ctx, (132, 9, 33), True, 24)
        torch.cuda.synchronize()
    finally:
        ctx.set_tuning(gradient_segment=0)


# ---- occupancy map and occupied-voxel count ------------------------------------------------------------------------------------------
OCCUPANCY_OFFSETS = [(0, 0, 0), (0, 1, 1), (2, 0, 2), (1, 3, 3), (4, 8, 0)]  # (d_volume, d_gradient, d_map)


def occupancy_scene(shape, block, variant):
    vol = T.random_volume(shape, seed=5, sparsity=0.97)
    if variant == "no_gradient":
        opt = abi.VolumeOptions(intensity_min=0.1, gradient_min=0.0, gradient_max=0.0)
    else:
        opt = abi.VolumeOptions(use_precomputed_gradient=(variant == "precomputed"), **T.APP_TF)
    scene = T.OracleScene(vol, opt, block)
    return scene, O.occupancy_map(scene.vol, scene.grad, scene.tex, scene.tf, block)


@pytest.mark.parametrize("shape,block", [((64, 9, 7), 4), ((68, 10, 6), 3), ((1028, 5, 3), 4)])
@pytest.mark.parametrize("variant", ["precomputed", "on_the_fly", "no_gradient"])
def test_occupancy_map_and_count(ctx, shape, block, variant):
    """vkv_occupancy_map and vkv_occupied_voxel_count: volume and gradient at different offsets from each other, the map at offsets 0 .. 3;
    (1028, 5, 3) gives several 64-dword spans per row.  d_count keeps the 8-byte alignment the ABI demands."""
    scene, expect = occupancy_scene(shape, block, variant)
    assert 0 < (expect == 0).mean() < 1, "test volume must give a mixed occupancy map"
    grad = scene.grad if scene.options.use_precomputed_gradient else None
    count = O.occupied_voxel_count(scene.vol, grad, scene.tf)
    d_tex = dev(scene.tex)
    for fill in FILLS:
        for vo, go, mo in OCCUPANCY_OFFSETS:
            what = "shape %s block %d %s volume +%d gradient +%d map +%d fill %#x" % (shape, block, variant, vo, go, mo, fill)
            d_vol, hv = G(scene.vol, vo, fill)
            d_grad, hg = G(grad, go, fill) if grad is not None else (None, None)
            d_map, hm = G(expect.shape, mo, fill)
            g_ptr = None if d_grad is None else d_grad.data_ptr()
            ctx.occupancy_map(d_vol.data_ptr(), g_ptr, d_tex.data_ptr(), scene.tf, scene.extent, d_map.data_ptr(), scene.map_extent, st())
            d_count = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
            ctx.occupied_voxel_count(d_vol.data_ptr(), g_ptr, scene.tf, scene.extent, d_count.data_ptr(), st())
            same(d_map, expect, what)
            assert int(d_count.item()) == count, what
            intact(what, volume=hv, map=hm, **({} if hg is None else {"gradient": hg}))


# ---- distance transforms -------------------------------------------------------------------------------------------------------------
# map extents (w, h, d).  y / z passes with width % XT == 0: XT 16; XT 8, SEG 256; XT 4, SEG 512; XT 8, SEG 768 and the chunked path
# (a line longer than 512 cells).  x pass: 8 and 16 cells per lane.  (12, 5, 3) is small enough for the brute-force statements.
DM_EXTENTS = [(32, 130, 5), (24, 300, 2), (8, 400, 3), (16, 600, 2), (260, 3, 4), (512, 4, 3), (1024, 2, 2), (12, 5, 3)]
ISO_OFFSETS = [(0, 0), (1, 0), (0, 2), (4, 0), (0, 8), (8, 4)]  # (d_map, d_swap)
# (eight octant maps, swap): all aligned; a fixed assignment that mixes them; only octant map 5 off by one; only map 7 (the occupancy, source
# of the x pass and its x- result) off by one; only map 3 (the x+ result) off by two - the x pass touches maps 3 and 7 alone, so its byte-row
# variant runs only when one of THEM is off
ANISO_OFFSETS = [((0,) * 8, 0), ((0, 1, 2, 5, 8, 3, 12, 18), 4), ((0, 0, 0, 0, 0, 1, 0, 0), 0), ((0, 0, 0, 0, 0, 0, 0, 1), 0), ((0, 0, 0, 2, 0, 0, 0, 0), 0)]


def dm_inputs(extent):
    w, h, d = extent
    shape = (d, h, w)
    sparse = sparse_occupancy(shape, 3, min(1.0, 6.0 / (w * h * d)))
    assert 0 < (sparse == 0).sum() < sparse.size
    rng = np.random.default_rng(w + h + d)
    raw = rng.integers(0, 256, size=shape, dtype=np.uint8)
    raw[rng.random(shape) < 0.7] = 255
    raw[rng.random(shape) < 0.01] = 0
    return [("sparse", sparse), ("bytes", raw)]


@pytest.mark.parametrize("extent", DM_EXTENTS, ids=["%dx%dx%d" % e for e in DM_EXTENTS])
def test_distance_map(ctx, extent):
    """vkv_distance_map in place in a guarded map with a guarded swap buffer, on a sparse 0 / 255 map and on arbitrary bytes."""
    w, h, d = extent
    for kind, occ in dm_inputs(extent):
        want = O.distance_map(occ)
        if kind == "sparse" and occ.size <= 3000:
            assert np.array_equal(want, T.brute_force_chebyshev(occ))
        for fill in FILLS:
            for mo, so in ISO_OFFSETS:
                what = "map %s %s map +%d swap +%d fill %#x" % (extent, kind, mo, so, fill)
                d_map, hm = G(occ, mo, fill)
                d_swap, hs = G(occ.shape, so, fill)
                ctx.distance_map(d_map.data_ptr(), d_swap.data_ptr(), abi.Extent3D(w, h, d), st())
                same(d_map, want, what)
                intact(what, map=hm, swap=hs)


@pytest.mark.parametrize("extent", DM_EXTENTS, ids=["%dx%dx%d" % e for e in DM_EXTENTS])
def test_distance_map_anisotropic(ctx, extent):
    """vkv_distance_map_anisotropic with the eight octant maps and the swap buffer each at their own offset: both launch plans (whole lines up
    to 512 cells - three launches, the z pass in place - and the 600-cell lines of (16, 600, 2))."""
    w, h, d = extent
    for kind, occ in dm_inputs(extent):
        want = O.distance_map_anisotropic(occ)
        if kind == "sparse" and occ.size <= 3000:
            for k in range(8):
                assert np.array_equal(want[k], T.brute_force_chebyshev_octant(occ, k)), "octant %d vs brute force" % k
        for fill in FILLS:
            for offs, so in ANISO_OFFSETS:
                what = "map %s %s maps +%s swap +%d fill %#x" % (extent, kind, list(offs), so, fill)
                pairs = [G(occ if k == 7 else occ.shape, offs[k], fill) for k in range(8)]
                d_swap, hs = G(occ.shape, so, fill)
                ctx.distance_map_anisotropic([m.data_ptr() for m, _ in pairs], d_swap.data_ptr(), abi.Extent3D(w, h, d), st())
                for k in range(8):
                    same(pairs[k][0], want[k], "%s: octant %d" % (what, k))
                intact(what, swap=hs, **{"map%d" % k: hk for k, (_, hk) in enumerate(pairs)})


# ---- map fills through the transfer-function updates ----------------------------------------------------------------------------------
def tf_update_volume(shape):
    """a volume whose occupancy map under APP_TF is mixed: noise below the window with a block of bright noise"""
    w, h, d = shape
    rng = np.random.default_rng(w)
    vol = rng.integers(0, 20, size=(d, h, w), dtype=np.uint8)
    vol[d // 2:, : h // 2, w // 3:] = rng.integers(60, 256, size=vol[d // 2:, : h // 2, w // 3:].shape, dtype=np.uint8)
    return vol


@pytest.mark.parametrize("from_summary", [False, True], ids=["update", "from_summary"])
@pytest.mark.parametrize("skip", [abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
@pytest.mark.parametrize("shape", [(12, 12, 8), (20, 16, 12)])  # block 4: maps of 3 x 3 x 2 = 18 and 5 x 4 x 3 = 60 cells
def test_map_fills_through_transfer_function_updates(ctx, shape, skip, from_summary):
    """vkv_update_transfer_function fills the map with k_fill_empty before the occupancy pass: maps of 18 and 60 cells at offsets 1, 7, 8, 15
    (and 0) from a 16-byte boundary - a head of 15 bytes, n hardly larger than the head, a body of 0 to 3 vectors.
    vkv_update_transfer_function_from_summary writes every cell from k_occupancy_from_summary, without that fill: the same maps at the same
    offsets check its stores and the transforms behind it.  Every map byte-equal to O.compute_distance_map, guards intact; d_tf and d_tables keep their 4-byte alignment."""
    vol = tf_update_volume(shape)
    opt = abi.VolumeOptions(use_precomputed_gradient=True, **T.APP_TF)
    scene = T.OracleScene(vol, opt, 4)
    want = scene.maps(skip)
    n_maps = 8 if skip == abi.SKIP_ANISOTROPIC_DISTANCE else 1
    assert want.shape[0] == n_maps
    assert 0 < (want[-1] == 0).mean() < 1, "test volume must give a mixed occupancy map"
    d_vol, d_grad = dev(scene.vol), dev(scene.grad)
    me = scene.map_extent
    cells = (me.depth, me.height, me.width)
    d_summary = None
    if from_summary:
        d_summary = torch.full((me.width * me.height * me.depth, abi.CELL_SUMMARY_BYTES), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.cell_summary(d_vol.data_ptr(), d_grad.data_ptr(), scene.extent, me, None, d_summary.data_ptr(), st())
    offsets = [1, 7, 8, 15, 0]
    for fill in FILLS:
        for i, off in enumerate(offsets):
            offs = [offsets[(i + k) % len(offsets)] for k in range(n_maps)]  # map 0 at `off`, the octant maps rotate through the list
            what = "shape %s skip %d maps +%s fill %#x" % (shape, skip, offs, fill)
            pairs = [G(cells, o, fill) for o in offs]
            d_swap, hs = G(cells, offsets[(i + 2) % len(offsets)], fill)
            d_tex = torch.full((256, 256, 4), 0x5A, dtype=torch.uint8, device="cuda")
            d_tab = torch.zeros(abi.TF_BITS_WORDS, dtype=torch.int32, device="cuda")
            args = [opt, d_vol.data_ptr(), d_grad.data_ptr(), scene.extent, d_tex.data_ptr(), d_tab.data_ptr(), [m.data_ptr() for m, _ in pairs],
                    d_swap.data_ptr(), me, skip, None]
            if from_summary:
                ctx.update_transfer_function_from_summary(*args, d_summary.data_ptr(), None, None, st())
            else:
                ctx.update_transfer_function(*args, st())
            for k in range(n_maps):
                same(pairs[k][0], want[k], "%s: map %d" % (what, k))
            intact(what, swap=hs, **{"map%d" % k: hk for k, (_, hk) in enumerate(pairs)})


# ---- vkv_convert_volume -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype,npt", [("uint8_t", "u1"), ("int8_t", "i1"), ("uint16_t", "u2"), ("int16_t", "i2")])
@pytest.mark.parametrize("endian", ["little", "big"])
def test_convert_volume(ctx, tmp_path, ctype, npt, endian):
    """vkv_convert_volume against the oracle's loader on the same file bytes: d_raw at every offset below 16 the ABI allows (any byte for 8-bit,
    even bytes for 16-bit voxels), d_out at 0, 1, 7, 8 - the per-element fallback for a whole volume, and the mixed case of an aligned source
    with a misaligned destination; n around one thread's 16 bytes, and 4099: more than one workgroup of 8-bit voxels, a partial last thread."""
    rng = np.random.default_rng(5)
    info = np.iinfo(npt)
    item = int(npt[1])
    lo, hi = (-20.0, 100.0) if item == 1 else (-400.0, 25380.0)
    for n in (1, 15, 16, 17, 4099):
        raw = rng.integers(info.min, info.max + 1, size=n).astype(npt)
        f = tmp_path / ("v%d.raw" % n)
        file_bytes = raw.astype(("<" if endian == "little" else ">") + npt)
        file_bytes.tofile(f)
        (tmp_path / ("v%d.raw.header" % n)).write_text("%d 1 1\n1 1 1\n%g %g\n%s %s\n1 0 0 0\n" % (n, lo, hi, ctype, endian))
        hdr = O.load_header(str(f) + ".header")
        expect = O.load_data(str(f), hdr).reshape(n)
        host_raw = np.frombuffer(file_bytes.tobytes(), np.uint8).copy()
        for fill in FILLS:
            for ro in range(0, 16, item):
                d_raw, hr = G(host_raw, ro, fill)
                for oo in (0, 1, 7, 8):
                    what = "%s %s n %d raw +%d out +%d fill %#x" % (ctype, endian, n, ro, oo, fill)
                    d_out, ho = G(n, oo, fill)
                    ctx.convert_volume(d_raw.data_ptr(), abi.VOXEL_TYPES[ctype], endian == "big", hdr.normalisation_range[0], hdr.normalisation_range[1], n,
                                       d_out.data_ptr(), st())
                    same(d_out, expect, what)
                    intact(what, out=ho)
                intact("%s %s n %d raw +%d fill %#x" % (ctype, endian, n, ro, fill), raw=hr)


# ---- vkv_update_volume_region -----------------------------------------------------------------------------------------------------------
def test_update_volume_region(ctx):
    """One state of test_gpu_volume_region.py's harness (shape (36, 20, 12), block 4, precomputed gradient, eight octant maps) with the volume, the
    gradient, every map and the swap buffer at mixed offsets, the packed image 256-byte aligned as required, the 16-bit source at +2: a single
    voxel, a box that touches x = 0 and the last column, the whole volume - everything byte-equal to the full rebuild on aligned copies."""
    shape, source = (36, 20, 12), SOURCES[2]  # uint16, big endian
    w, h, d = shape
    base = dev(T.random_volume(shape, 36, sparsity=0.5))
    map_offsets = [1, 0, 2, 4, 8, 3, 15, 7]
    for fill in FILLS:
        rng = np.random.default_rng(36)
        s = State(ctx, base, 4, T.APP_TF, "precomputed", True, abi.SKIP_ANISOTROPIC_DISTANCE)
        handles = {}

        def move(name, t, off):
            view, handles[name] = G(t, off, fill)
            return view

        s.vol, s.grad, s.packed = move("volume", s.vol, 1), move("gradient", s.grad, 3), move("packed", s.packed, 0)
        s.maps = [move("map%d" % k, m, map_offsets[k]) for k, m in enumerate(s.maps)]
        s.swap = move("swap", s.swap, 5)
        assert s.packed.data_ptr() % 256 == 0
        exp = s.vol.clone()
        for box in (abi.Box(18, 10, 6, 1, 1, 1), abi.Box(0, 5, 3, w, 4, 3), abi.Box(0, 0, 0, w, h, d)):
            what = "box %s fill %#x" % ((box.x0, box.y0, box.z0, box.width, box.height, box.depth), fill)
            src = make_source(rng, source, box, empty_share=0.5)
            d_src, handles["source"] = G(src, 2, fill)
            exp = expected_volume(ctx, exp, src, source, box)
            s.update(d_src, source, box)
            bad = mismatches(s, exp)
            assert not bad, "%s: %s" % (what, ", ".join(bad))
            intact(what, **handles)


# ---- vkv_pack_volume --------------------------------------------------------------------------------------------------------------------
PACK_OFFSETS = [(0, 0), (0, 1), (2, 0), (1, 2), (3, 3)]  # (d_volume, d_gradient)


@pytest.mark.parametrize("with_gradient", [True, False])
@pytest.mark.parametrize("shape", [(64, 9, 6), (68, 9, 6), (67, 9, 6)])
def test_pack_volume(ctx, shape, with_gradient):
    """k_pack_volume_tiled<., ALIGNED>: the packed image, every padding byte included, equals the image packed from aligned copies into a
    buffer with the same pre-fill (test_packed_image_of_misaligned_inputs_renders_the_oracle_frame pins the image to the oracle)."""
    vol = T.random_volume(shape, seed=17)
    grad = T.random_volume(shape, seed=18) if with_gradient else None  # the pack interleaves bytes: any gradient bytes do
    ext = abi.Extent3D(*shape)
    n = ctx.packed_volume_bytes(ext)
    a_vol, a_grad = dev(vol), None if grad is None else dev(grad)
    for fill in FILLS:
        want = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
        ctx.pack_volume(a_vol.data_ptr(), None if a_grad is None else a_grad.data_ptr(), ext, want.data_ptr(), st())
        want = want.cpu().numpy()
        assert (want != fill).any()
        for vo, go in PACK_OFFSETS:
            what = "shape %s gradient %s volume +%d gradient +%d fill %#x" % (shape, with_gradient, vo, go, fill)
            d_vol, hv = G(vol, vo, fill)
            d_grad, hg = G(grad, go, fill) if grad is not None else (None, None)
            d_packed, hp = G(n, 0, fill)
            ctx.pack_volume(d_vol.data_ptr(), None if d_grad is None else d_grad.data_ptr(), ext, d_packed.data_ptr(), st())
            same(d_packed, want, what)
            intact(what, volume=hv, packed=hp, **({} if hg is None else {"gradient": hg}))


def test_packed_image_of_misaligned_inputs_renders_the_oracle_frame(ctx):
    """A 96 x 64 TEST_NUM_TEXTURE_SAMPLES frame and its RGBA8 sampled from the image packed from a volume at +1 and a gradient at +2 (width 68:
    the pointers alone make it the unaligned template) equal OracleScene.render: an independent statement of the image, not its sibling."""
    scene = T.OracleScene(O.synth_volume((68, 56, 48), 1, 21), abi.VolumeOptions(**T.APP_TF), 4)
    v, tf = make_gpu_volume(ctx, scene)
    V.ComputeDistanceMap(ctx).compute(v, tf, abi.SKIP_DISTANCE)
    size = (96, 64)
    view, proj = T.orbit(60.0, image_size=size)
    opts = abi.RenderOptions(skipping_type=abi.SKIP_DISTANCE, clip_distance=1.0, early_ray_termination=False, test=abi.TEST_NUM_TEXTURE_SAMPLES)
    params = scene.params(view, proj, size, opts)
    ref = scene.render(params, want_rgba8=True)
    assert ref.counts[..., 0].sum() > 0
    sp = V.VolumeRenderSubpass(ctx, v, opts, size)
    for fill in FILLS:
        d_vol, hv = G(scene.vol, 1, fill)
        d_grad, hg = G(scene.grad, 2, fill)
        d_packed, hp = G(ctx.packed_volume_bytes(scene.extent), 0, fill)
        ctx.pack_volume(d_vol.data_ptr(), d_grad.data_ptr(), scene.extent, d_packed.data_ptr(), st())
        p = sp.bind(params)
        assert p.d_packed_volume and p.d_transfer_function_bits
        p.d_packed_volume = d_packed.data_ptr()
        color = torch.full((size[1], size[0], 4), -1.0, dtype=torch.float32, device="cuda")
        rgba8 = torch.full((size[1], size[0], 4), fill, dtype=torch.uint8, device="cuda")
        counts = torch.full((size[1], size[0], 3), 0xFFFF, dtype=torch.int32, device="cuda")
        sp.draw(p, color, rgba8, counts)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy().astype(np.uint32), ref.counts)
        assert np.array_equal(color.cpu().numpy(), ref.color)  # the count's grey level: exact
        same(rgba8, ref.rgba8, "RGBA8, fill %#x" % fill)
        intact("fill %#x" % fill, volume=hv, gradient=hg, packed=hp)


# ---- vkv_scatter_tiles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp,offsets", [(4, [(0, 0), (4, 0), (0, 8), (4, 4), (8, 8), (12, 12)]), (16, [(0, 0), (16, 16), (16, 0)])])
def test_scatter_tiles(ctx, bpp, offsets):
    """The de-interleave of three ranks' tiles of a rectangle smaller than the 80 x 48 image against numpy: RGBA8 with the image and the gathered
    buffer at +4, +8, +12 - one pixel per thread at a width that is a multiple of 4 - and 16-byte pixels at +16."""
    world, size, tile = 3, (80, 48), 16
    rect = abi.TileRect(1, 0, 3, 3)
    tpr = -(-(rect.w * rect.h) // world)
    flat = np.random.default_rng(bpp).integers(0, 256, size=(world, tpr * tile * tile, bpp), dtype=np.uint8)
    want = multigpu.deinterleave_reference(flat, size, tile, world, rect)
    assert want.any() and not want[:, :tile].any()
    for fill in FILLS:
        for io, so in offsets:  # (d_image, d_gathered)
            what = "bpp %d image +%d gathered +%d fill %#x" % (bpp, io, so, fill)
            d_flat, hf = G(flat, so, fill)
            d_img, hi = G((size[1], size[0], bpp), io, fill)
            ctx.scatter_tiles(d_flat.data_ptr(), d_img.data_ptr(), size, (tile, tile), world, tpr, bpp, st(), rect=rect)
            same(d_img, want, what)
            intact(what, image=hi, gathered=hf)


# ---- integrator output ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_scene(ctx):
    scene = T.OracleScene(O.synth_volume((64, 56, 48), 1, 9), abi.VolumeOptions(**T.APP_TF), 4)
    v, tf = make_gpu_volume(ctx, scene)
    V.ComputeDistanceMap(ctx).compute(v, tf, abi.SKIP_DISTANCE)
    return scene, v


@pytest.mark.parametrize("width", [208, 210])
def test_integrator_rgba8_target(ctx, frame_scene, width):
    """vkv_render and vkv_render_batch through the frame's tile rectangle with fill_outside, d_out_rgba8 the only output, at +4 (and +0): the
    launch clears the tiles outside the rectangle with 16-byte stores only when the target and the rows allow it.  The frame equals the
    oracle's RGBA8 with the guards around the target intact.  (The only test here that launches the ray-march kernels; it adds nothing to them.)"""
    scene, v = frame_scene
    size = (width, 96)
    view, proj = T.orbit(25.0, image_size=size)
    opts = abi.RenderOptions(skipping_type=abi.SKIP_DISTANCE, clip_distance=1.0)
    p0 = scene.params(view, proj, size, opts)
    rect = lib.screen_tile_rect(p0.ray_cast, p0.ray_gen, size, (16, 16))
    assert 0 < rect.tiles < (-(-width // 16)) * 6, "the rectangle must leave tiles outside it"
    pf = abi.RenderParams.from_buffer_copy(p0)
    pf.tiles = abi.full_frame_tiles(size[0], size[1], 16, 16, rect=rect, fill_outside=True)
    assert pf.tiles.fill_outside == 1
    ref = scene.render(pf, want_rgba8=True)
    assert ref.rgba8.any()
    sp = V.VolumeRenderSubpass(ctx, v, opts, size)
    for fill in FILLS:
        for off in (4, 0):
            what = "width %d target +%d fill %#x" % (width, off, fill)
            targets = [G((size[1], size[0], 4), off, fill) for _ in range(3)]
            qs = []
            for t, _ in targets:
                q = sp.bind(pf)
                q.d_out_color, q.d_out_rgba8, q.d_out_counts, q.d_out_depth, q.d_in_depth, q.blend_over_target = None, t.data_ptr(), None, None, None, 0
                qs.append(q)
            ctx.render(qs[0], st())
            ctx.render_batch(qs[1:], st())
            torch.cuda.synchronize()
            for name, (t, h) in zip(("vkv_render", "vkv_render_batch frame 0", "vkv_render_batch frame 1"), targets):
                same(t, ref.rgba8, "%s: %s" % (what, name))
                intact("%s: %s" % (what, name), target=h)
