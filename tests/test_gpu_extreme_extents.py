"""GPU: the ray-marcher against the oracle at needle, slab and one-voxel extents (the case table and what it stands on: tests/test_extreme_extents_cpu.py).

Per case: gradient map, the maps of every skipping type, then the frame of every skipping type - packed / linear sampling x tile / persistent
scheduler with equal bits (gpu_render), counters exact, colour and depth within test_gpu_parity's COLOR_TOL / DEPTH_TOL.  Needles also with the
two-level tables and the register arithmetic forced (same bits as the default) and without a counter buffer.  Mixed batches through
vkv_render_batch: every frame the bits of its own vkv_render.

Which address-table kind a launch took, and whether a batch kept one kernel or fell back to register arithmetic, is inferred from the launcher's
documented rule (restated in test_extreme_extents_cpu.py); there is no accessor for it."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests import test_extreme_extents_cpu as X
from tests.test_gpu_parity import compare_render, gpu_render, make_gpu_volume
from vkvolume_amd import abi, volume as V

pytestmark = pytest.mark.gpu
FIELDS = ("color", "rgba8", "depth", "counts")


def frame_buffers(with_counts=True):
    w, h = X.SIZE
    return dict(color=torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda"), rgba8=torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda"),
                depth=torch.full((h, w), -1.0, dtype=torch.float32, device="cuda"),
                counts=torch.full((h, w, 3), 0xFFFF, dtype=torch.int32, device="cuda") if with_counts else None)


def point(p, o):
    q = abi.RenderParams.from_buffer_copy(p)
    q.d_out_color, q.d_out_rgba8, q.d_out_depth = o["color"].data_ptr(), o["rgba8"].data_ptr(), o["depth"].data_ptr()
    q.d_out_counts = o["counts"].data_ptr() if o["counts"] is not None else None
    q.d_in_depth, q.blend_over_target = None, 0
    return q


def same_frame(a, b, what, fields=FIELDS):
    for k in fields:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


# ---- 1. every case against the oracle, 2. the table kinds on the needles ---------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_case_matches_the_oracle(ctx, case):
    scene = X.build_scene(case)
    name = X.case_id(case)
    v, tf = make_gpu_volume(ctx, scene)
    if scene.options.use_precomputed_gradient:
        assert np.array_equal(v.gradient.cpu().numpy(), scene.grad), name + ": gradient map"
    cdm = V.ComputeDistanceMap(ctx)
    st_ = torch.cuda.current_stream().cuda_stream
    for st in X.SKIPS:
        cdm.compute(v, tf, st)
        expect = scene.maps(st)
        for k in range(expect.shape[0]):
            assert np.array_equal(v.distance_maps[k].cpu().numpy(), expect[k]), "%s: map %d of skipping type %d" % (name, k, st)
        for ert in ((True, False) if X.both_ert(case) else (True,)):
            label = "%s mode %d ert %d" % (name, st, ert)
            params = X.case_params(scene, case, st, ert)
            ref = scene.render(params, want_rgba8=True)
            got = gpu_render(ctx, v, params, want_rgba8=True)
            compare_render(got, ref, label)
            assert np.array_equal(got[3], ref.rgba8), label + ": RGBA8"
            if not X.is_needle(case):
                continue
            # the frame above (default tuning: per-voxel tables up to W + H + D = 3446, two-level tables beyond) against the other kinds
            default = dict(color=got[0], counts=got[1].astype(np.int32), depth=got[2], rgba8=got[3])
            sp = V.VolumeRenderSubpass(ctx, v, params.options, X.SIZE)
            p = sp.bind(params)
            assert bool(p.d_packed_volume)
            try:
                for tables in (2, 1, 0):
                    ctx.set_tuning(address_tables=tables)
                    counted, plain = frame_buffers(), frame_buffers(with_counts=False)
                    ctx.render(point(p, counted), st_)
                    ctx.render(point(p, plain), st_)
                    torch.cuda.synchronize()
                    for k in FIELDS:
                        assert np.array_equal(counted[k].cpu().numpy(), default[k]), "%s, address_tables %d: %s differs from the default frame" % (label, tables, k)
                    same_frame(plain, counted, "%s, address_tables %d, no counter buffer" % (label, tables), FIELDS[:3])
            finally:
                ctx.set_tuning(address_tables=2)


# ---- 3. mixed batches -------------------------------------------------------------------------------------------------------------------------
VIEWS = X.BATCH_VIEWS


BATCH_RUNS = [(b, 0) for b in X.BATCHES] + [(b, 1) for b in X.BATCHES if b[0] == "c-needle-and-cube"]        # (d): (c) with the pull switch


@pytest.mark.parametrize("batch,batch_mode", BATCH_RUNS, ids=["%s-mode%d" % (b[0], m) for b, m in BATCH_RUNS])
def test_mixed_batch_equals_single_launches(ctx, batch, batch_mode):
    """Frames of volumes of different extents in one vkv_render_batch: two views of each volume, the volumes alternating.  batch_mode 1 asks for
    the pull kernel, which must not be taken for frames of different volumes: the same bits."""
    name, vols, shared = batch
    assert X.batch_shares_a_kernel([e for e, _, _ in vols]) == shared
    what = "%s (%s by the launcher's rule)" % (name, "one kernel, each workgroup its own frame's tables" if shared else "register fallback")
    scenes = [X.build_scene((whd, voxel, block) + VIEWS[0]) for whd, voxel, block in vols]
    dvols = [make_gpu_volume(ctx, s) for s in scenes]
    st_ = torch.cuda.current_stream().cuda_stream
    for st in X.SKIPS:
        for v, tf in dvols:
            V.ComputeDistanceMap(ctx).compute(v, tf, st)
        frames = []
        for az, el in VIEWS:
            for scene, (whd, voxel, block), (v, tf) in zip(scenes, vols, dvols):
                params = X.case_params(scene, (whd, voxel, block, az, el), st)
                frames.append((scene, params, V.VolumeRenderSubpass(ctx, v, params.options, X.SIZE).bind(params)))
        for with_counts in (True, False):
            single = [frame_buffers(with_counts) for _ in frames]
            batched = [frame_buffers(with_counts) for _ in frames]
            for (_, _, p), o in zip(frames, single):
                ctx.render(point(p, o), st_)
            ctx.set_tuning(batch_mode=batch_mode)
            try:
                ctx.render_batch([point(p, o) for (_, _, p), o in zip(frames, batched)], st_)
                torch.cuda.synchronize()
            finally:
                ctx.set_tuning(batch_mode=0)
            for i, (a, b) in enumerate(zip(single, batched)):
                same_frame(b, a, "%s, mode %d, counters %d, frame %d: batch against the single launch" % (what, st, with_counts, i), FIELDS if with_counts else FIELDS[:3])
            if with_counts:
                for i in (0, 3):        # a frame of each volume against the oracle
                    scene, params, _ = frames[i]
                    o = batched[i]
                    got = (o["color"].cpu().numpy(), o["counts"].cpu().numpy().astype(np.uint32), o["depth"].cpu().numpy(), None)
                    ref = scene.render(params)
                    assert int(ref.counts[..., 0].sum()) > 0 and float(ref.color[..., 3].max()) > 0.0
                    compare_render(got, ref, "%s, mode %d, frame %d" % (what, st, i))


# ---- 4. the direct renderers ------------------------------------------------------------------------------------------------------------------
# (extent, voxel size, block, views): the one-voxel slabs, the column and one needle per axis; the needles also along their long axis
DIRECT_SIZE = (24, 16)
DIRECT = [
    ((1, 40, 30), (30, 1, 1), 4, ((70.0, 15.0),)),
    ((2, 3, 300), (150, 100, 1), 4, ((33.0, 20.0), (0.0, 0.0))),
    ((1, 257, 129), (100, 1, 1), 4, ((70.0, 20.0),)),
    ((1011, 4, 4), (4.0 / 1011, 1, 1), 2, ((33.0, 20.0), (90.0, 0.0))),
    ((4, 2035, 4), (1, 4.0 / 2035, 1), 3, ((33.0, 20.0), (0.0, 89.0))),
    ((4, 3, 3060), (1, 1, 4.0 / 3060), 4, ((33.0, 20.0), (0.0, 0.0))),
]
DIRECT_IDS = ["%dx%dx%d" % d[0] for d in DIRECT]


def direct_volume(whd):
    return T.random_volume(whd, 4000 + sum(whd), sparsity=0.9)


@pytest.mark.parametrize("whd,voxel,block,views", DIRECT, ids=DIRECT_IDS)
def test_mip_and_isosurface_match_their_statements(ctx, whd, voxel, block, views):
    """draw_mip and draw_iso: the dense frame against mip_np / iso_np bit for bit, the max-map frame against the dense one bit for bit, with the
    packed and the linear layout"""
    from tests import test_gpu_iso as GI, test_gpu_mip as GM
    from tests.test_iso_cpu import iso_np, iso_options
    from tests.test_mip_cpu import max_map_np, mip_np, rays_np, samples_np
    vol = direct_volume(whd)
    thr, wmax, iso = 0.15, 0.8, iso_options(0.3, 4)
    found_mip = found_iso = skipped = 0
    refs = {}
    for packed in (True, False):
        v = GI.make_volume(ctx, vol, block=block, packed=packed, voxel_size=voxel)
        me = v.map_extent
        assert np.array_equal(v.max_map.cpu().numpy(), max_map_np(vol, (me.width, me.height, me.depth)))
        for az, el in views:
            what = (whd, packed, az, el)
            sp, p = GI.subpass(v, az, el, X.RADIUS, size=DIRECT_SIZE)
            if packed:        # (the statements do not depend on the layout)
                S = samples_np(vol, rays_np(p))
                refs[(az, el)] = (mip_np(p, vol, abi.MipOptions(threshold=thr, window_max=wmax), S=S), iso_np(p, vol, iso, S=S))
                found_mip += int(refs[(az, el)][0]["found"].sum())
                found_iso += int(refs[(az, el)][1]["found"].sum())
            ref_mip, ref_iso = refs[(az, el)]
            dense = GM.draw(sp, p, thr, wmax, skip=False, size=DIRECT_SIZE)
            GM.assert_matches_numpy(dense, ref_mip, what)
            fast = GM.draw(sp, p, thr, wmax, skip=True, size=DIRECT_SIZE)
            GM.assert_same_bits(fast, dense, what)
            skipped += int(fast["counts"][:, 2].sum())
            dense = GI.draw(sp, p, iso.iso, skip=False, size=DIRECT_SIZE, **GI.kw_of(iso))
            GI.assert_matches_numpy(dense, ref_iso, what)
            fast = GI.draw(sp, p, iso.iso, skip=True, size=DIRECT_SIZE, **GI.kw_of(iso))
            GI.assert_same_bits(fast, dense, what)
            skipped += int(fast["counts"][:, 2].sum())
    assert found_mip >= 40 * len(views) and found_iso >= 40 * len(views) and skipped > 0, (found_mip, found_iso, skipped)


def direct_planes(whd):
    """two planes in texture coordinates (pixel (x, y), sample j at origin + x du + y dv + j dn), both a little larger than the volume so that
    pixels and samples fall outside it: 'through' looks along the longest axis with one sample per voxel of it (4096 at the most) and a slight
    tilt, 'lengthwise' lays the longest axis across the image's width and samples across the shortest axis"""
    w, h = DIRECT_SIZE
    order = np.argsort(whd, kind="stable")
    thin, mid, lng = (int(a) for a in order)
    vec = lambda **kw: np.array([kw.get("xyz"[a], 0.0) for a in range(3)], np.float32)  # noqa: E731
    ax = "xyz"
    ns = min(4096, whd[lng] + 8)
    through = dict(origin=vec(**{ax[mid]: -0.1, ax[thin]: -0.1, ax[lng]: -0.001}), du=vec(**{ax[mid]: 1.2 / (w - 1)}), dv=vec(**{ax[thin]: 1.2 / (h - 1)}),
                   dn=vec(**{ax[lng]: 1.002 / (ns - 1), ax[mid]: 0.1 / (ns - 1)}), samples=ns)
    ns = 9
    lengthwise = dict(origin=vec(**{ax[lng]: -0.05, ax[mid]: -0.1, ax[thin]: -0.2}), du=vec(**{ax[lng]: 1.1 / (w - 1)}), dv=vec(**{ax[mid]: 1.2 / (h - 1)}),
                      dn=vec(**{ax[thin]: 1.4 / (ns - 1), ax[lng]: 0.01 / (ns - 1)}), samples=ns)
    return (("through", through), ("lengthwise", lengthwise))


@pytest.mark.parametrize("whd,voxel,block,views", DIRECT, ids=DIRECT_IDS)
def test_slab_matches_its_statement(ctx, whd, voxel, block, views):
    """draw_slab: every mode dense against slab_np, SLAB_MAX over the max map against slab_skip_np (counters included), bit for bit, with the
    packed and the linear layout"""
    from tests import test_gpu_slab as GS
    from tests.test_mip_cpu import max_map_np
    from tests.test_slab_cpu import MODES, slab_np, slab_options, slab_samples_np, slab_skip_np
    vol = direct_volume(whd)
    refs, counted, skipped = {}, 0, 0
    for packed in (True, False):
        v = GS.make_volume(ctx, vol, block=block, packed=packed)
        me = (v.map_extent.width, v.map_extent.height, v.map_extent.depth)
        mm = max_map_np(vol, me)
        assert np.array_equal(v.max_map.cpu().numpy(), mm)
        sp, p = GS.bound(v, DIRECT_SIZE)
        for name, plane in direct_planes(whd):
            o = slab_options(plane, window=(0.05, 0.7))
            if packed:
                S = slab_samples_np(p, vol, o)
                dense = {}
                for mode in MODES:
                    o.mode = mode
                    dense[mode] = slab_np(p, vol, o, S)
                o.mode = abi.SLAB_MAX
                refs[name] = (dense, slab_skip_np(p, vol, mm, o, S))
                counted += int(dense[abi.SLAB_MAX]["count"].sum())
                skipped += int(refs[name][1]["counts"][:, 2].sum())
                assert (dense[abi.SLAB_MAX]["count"] == 0).any() and (dense[abi.SLAB_MAX]["count"] > 0).sum() >= 40, (whd, name)
            dense, fast = refs[name]
            for mode in MODES:
                o.mode = mode
                GS.assert_matches(GS.draw(sp, p, o, skip=False), dense[mode], (whd, packed, name, mode, "dense"))
            o.mode = abi.SLAB_MAX
            GS.assert_matches(GS.draw(sp, p, o, skip=True), fast, (whd, packed, name, "skip"), counts=fast["counts"])
    assert counted > 1000 and skipped > 0, (counted, skipped)
