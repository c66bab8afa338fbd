"""GPU: the host-side state vkv_render / vkv_render_batch keep between calls - the opacity-correction tables cached by (voxel_alpha_factor,
sampling_factor) and the pinned ring the batch launcher assembles its argument upload in - never changes a frame: every frame is compared
with the CPU oracle, sample counters and RGBA8 bit for bit."""
import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_gpu_parity import make_gpu_volume
from vkvolume_amd import abi, volume as V

pytestmark = pytest.mark.gpu
SIZE = (96, 64)
SKIP = abi.SKIP_DISTANCE


@pytest.fixture(scope="module")
def scene(ctx):
    sc = T.OracleScene(O.synth_volume((64, 56, 48), 1, 0xA1FA), abi.VolumeOptions(**T.APP_TF), 4)
    v, tf = make_gpu_volume(ctx, sc)
    V.ComputeDistanceMap(ctx).compute(v, tf, SKIP)
    ro = abi.RenderOptions(skipping_type=SKIP, clip_distance=1.0)
    return sc, V.VolumeRenderSubpass(ctx, v, ro, SIZE), ro


def _params(scene, azimuth, sampling_factor, voxel_alpha_factor):
    sc, sp, ro = scene
    view, proj = T.orbit(azimuth, image_size=SIZE)
    p = sp.bind(sc.params(view, proj, SIZE, ro))
    p.transfer_function.sampling_factor = sampling_factor
    p.transfer_function.voxel_alpha_factor = voxel_alpha_factor
    return p


def _outputs(p):
    o = dict(counts=torch.full((SIZE[1], SIZE[0], 3), 9, dtype=torch.int32, device="cuda"),
             rgba8=torch.full((SIZE[1], SIZE[0], 4), 7, dtype=torch.uint8, device="cuda"))
    p.d_out_color, p.d_out_depth = None, None
    p.d_out_counts, p.d_out_rgba8 = o["counts"].data_ptr(), o["rgba8"].data_ptr()
    return o


def _check(scene, p, o, label):
    ref = scene[0].render(p, want_rgba8=True)
    assert ref.counts[..., 0].sum() > 0, "%s: the oracle's frame is empty" % label
    assert np.array_equal(o["counts"].cpu().numpy().astype(np.uint32), ref.counts), "%s: sample counters differ from the oracle" % label
    assert np.array_equal(o["rgba8"].cpu().numpy(), ref.rgba8), "%s: RGBA8 differs from the oracle" % label


# two sampling factors x two opacity factors, visited so that every key comes back after the others were used (a stale entry would show)
KEYS = [(1.0, 1.0), (2.5, 1.0), (1.0, 0.35), (2.5, 0.35), (1.0, 1.0), (2.5, 0.35), (1.0, 0.35), (2.5, 1.0)]


def test_alternating_transfer_function_factors_render_the_oracles_frames(ctx, scene):
    st = torch.cuda.current_stream().cuda_stream
    # single launches
    done = []
    for k, (sf, vaf) in enumerate(KEYS):
        p = _params(scene, 25.0 * k, sf, vaf)
        o = _outputs(p)
        ctx.render(p, st)
        done.append((p, o, "vkv_render %d (sampling %g, alpha %g)" % (k, sf, vaf)))
    # batches with the keys mixed inside one launch, twice (the second launch finds every key cached)
    for rep in range(2):
        plist, outs = [], []
        for k, (sf, vaf) in enumerate(KEYS):
            p = _params(scene, 40.0 * k + 7.0 * rep, sf, vaf)
            outs.append(_outputs(p))
            plist.append(p)
        ctx.render_batch(plist, st)
        done += [(p, o, "vkv_render_batch %d frame %d (sampling %g, alpha %g)" % (rep, k, *KEYS[k])) for k, (p, o) in enumerate(zip(plist, outs))]
    # more keys than the cache holds, then the first ones again
    many = [(1.0 + 0.25 * k, 1.0 - 0.05 * k) for k in range(12)] + KEYS[:3]
    for k, (sf, vaf) in enumerate(many):
        p = _params(scene, 11.0 * k, sf, vaf)
        o = _outputs(p)
        ctx.render(p, st)
        done.append((p, o, "vkv_render, key %d of many (sampling %g, alpha %g)" % (k, sf, vaf)))
    torch.cuda.synchronize()
    for p, o, label in done:
        _check(scene, p, o, label)


def test_many_batch_launches_in_flight_on_one_stream_keep_their_arguments(ctx, scene):
    """64 launches on one stream with no synchronise in between, each with other cameras: a launch whose argument blocks were overwritten
    before its upload had read them would render another launch's view."""
    st = torch.cuda.current_stream().cuda_stream
    done = []
    for k in range(64):
        plist, outs = [], []
        for j, (sf, vaf) in enumerate(((1.0, 1.0), (2.5, 0.35))):
            p = _params(scene, 5.5 * k + 2.0 * j, sf, vaf)
            outs.append(_outputs(p))
            plist.append(p)
        ctx.render_batch(plist, st)
        done += [(p, o, "launch %d frame %d" % (k, j)) for j, (p, o) in enumerate(zip(plist, outs))]
    torch.cuda.synchronize()
    for p, o, label in done:
        _check(scene, p, o, label)
