"""vkv_distance_transform, vkv_distance_transform_weighted and vkv_nearest_target held to each other and to the numpy statements across every
pass schedule: x alone, x and y, x and z, all three, and a row longer than one bit word.  The three calls share the row walk, the envelope
pass and the schedule of vkvolume_amd/csrc/edt_passes.hpp (k_near_x with a copy of the walk); with weights (1, 1, 1) their distances are the same bytes.  The calls run through
the guarded run() of each call's own test file."""
import numpy as np
import pytest
import torch

from tests.test_distance_cpu import TO_INSIDE, TO_OUTSIDE, edt2_np
from tests.test_distance_weighted_cpu import edt2_weighted_np
from tests.test_gpu_components import same
from tests.test_gpu_distance import ISO, contents, run as run_unweighted, upload
from tests.test_gpu_distance_weighted import run as run_weighted
from tests.test_gpu_nearest import run as run_nearest
from tests.test_nearest_cpu import nearest_separable_np
from vkvolume_amd import lib

pytestmark = pytest.mark.gpu

EXTENTS = [(9, 1, 1), (9, 5, 1), (9, 1, 5), (9, 5, 5), (70, 3, 2)]        # (width, height, depth): (y runs, z runs) in all four ways; 70 > 64
CONTENTS = ("random 0.5", "corner 0", "no target")
LIMITS = (None, 10)


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


def make(content, shape_dhw, seed):
    return np.full(shape_dhw, 17, np.uint8) if content == "no target" else contents(content, shape_dhw, seed)


@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_the_three_calls_agree_with_each_other_and_the_statements(ctx, extent):
    w, h, d = extent
    for k, content in enumerate(CONTENTS):
        vol = make(content, (d, h, w), seed=900 + k)
        device_volume = upload(vol)
        for target in (TO_INSIDE, TO_OUTSIDE):
            for limit in LIMITS:
                what = "%s %s, to %s, limit %s" % (content, extent, ("inside", "outside")[target], limit)
                kw = dict(device_volume=device_volume, what=what)
                # weights (1, 1, 1): three calls, one set of bytes
                plain = run_unweighted(ctx, vol, ISO, target, limit, **kw)
                weighted = run_weighted(ctx, vol, ISO, target, (1, 1, 1), limit, **kw)
                nearest, dist2 = run_nearest(ctx, vol, ISO, target, (1, 1, 1), limit, **kw)
                same(plain, edt2_np(vol, ISO, target, limit), what + ": vkv_distance_transform against edt2_np")
                assert plain.tobytes() == weighted.tobytes(), what + ": vkv_distance_transform_weighted with unit weights"
                assert plain.tobytes() == dist2.tobytes(), what + ": vkv_nearest_target's d_dist2 with unit weights"
                same(nearest, nearest_separable_np(vol, ISO, (1, 1, 1), target, limit)[0], what + ": d_nearest")
                # weights (2, 2, 5): the two weighted calls
                weighted = run_weighted(ctx, vol, ISO, target, (2, 2, 5), limit, **kw)
                nearest, dist2 = run_nearest(ctx, vol, ISO, target, (2, 2, 5), limit, **kw)
                same(weighted, edt2_weighted_np(vol, ISO, (2, 2, 5), target, limit), what + ": weights (2, 2, 5) against edt2_weighted_np")
                assert dist2.tobytes() == weighted.tobytes(), what + ": d_dist2 against the weighted call, weights (2, 2, 5)"
                same(nearest, nearest_separable_np(vol, ISO, (2, 2, 5), target, limit)[0], what + ": d_nearest, weights (2, 2, 5)")
