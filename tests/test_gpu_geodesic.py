"""GPU: vkv_geodesic_propagate bit for bit against the numpy statements of tests/test_geodesic_cpu.py, after resumed
calls until d_counts[0] == 1, and Volume.geodesic_propagate / grow_from_points / split_bodies against them.

The extents lie around the tile edge of 8 (and around 16, should the tile grow), with axes of length 1, and 70 x 66 x 65 is several hundred
tiles.  Contents: the ones BUILT FOR TIES (seeds mirrored about the middle plane of an odd axis, in both memory orders; a checkerboard of
seeds; label 0xffffffff against label 1) and random masks of three densities with random seeds; every step table and five limits.  The
reference of a limited call is the unlimited one cut at the limit, which tests/test_geodesic_cpu.py proves to be the definition.  Tile seams:
diagonal staircases through tile corners, a serpentine and a needle driven one round per call (the resume path; the needle is 25 tiles
long).  Every buffer is a tests/helpers.py guarded() allocation, pre-filled and compared as a whole; the scratch is exactly
geodesic.scratch_bytes()."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_geodesic_cpu import (BIG_STEPS, CHAMFER, NONE, SPACING_STEPS, STEPS_6, STEPS_26, TABLES, checkerboard_seeds, crop, extreme_labels, gap_scene,
                                     geodesic_np, geodesic_sweeps_np, mirrored_seeds, serpentine, split_bodies_geodesic_np, staircase)
from tests.test_gpu_components import same
from tests.test_gpu_distance import contents, upload
from tests.test_gpu_mesh import FILL, ISO, ext_of, st
from tests.test_gpu_mesh_indexed import guard_damage
from tests.test_gpu_mip import make_volume
from tests.test_nearest_cpu import bridge_scene, split_bodies_np
from vkvolume_amd import abi, geodesic, lib

pytestmark = pytest.mark.gpu

EXTENTS = [(1, 1, 1), (1, 1, 9), (9, 1, 1), (1, 9, 1), (3, 5, 7), (8, 8, 8), (9, 9, 9), (16, 8, 8), (17, 9, 10), (33, 17, 9), (63, 1, 2), (64, 2, 1),
           (65, 3, 2)]        # (width, height, depth)


def limits_of(steps):
    return (None, 1, min(c for c in steps if c), 20, 100000)


def cut(dist, labels, limit):
    """the limited call's outputs from the unlimited ones"""
    if limit is None:
        return dist, labels
    keep = dist < np.uint32(min(limit, NONE))
    return np.where(keep, dist, np.uint32(NONE)), np.where(keep, labels, np.uint32(0))


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


# ---- one propagation ------------------------------------------------------------------------------------------------------------------------
def run(ctx, vol, seeds, steps, limit, box=None, rounds=64, device_volume=None, want_dist=True, want_labels=True, in_place=False, max_calls=40, what=""):
    """(d_dist, d_labels, reached, trace): the whole output buffers of the box's shape (uint32; None where not asked for), d_counts[1] and
    the d_counts[0] of every call, of ONE vkv_geodesic_propagate call of `rounds` rounds and resumed calls of as many until d_counts[0] is 1,
    on guarded buffers, every output, the scratch and the counts pre-filled with FILL; in_place: d_labels is d_seeds"""
    abox = None if box is None else abi.Box(*box)
    shape = vol.shape if box is None else (box[5], box[4], box[3])
    n = int(np.prod(shape))
    w, h, d = shape[2], shape[1], shape[0]
    d_vol, h_vol = upload(vol) if device_volume is None else device_volume
    nbytes = geodesic.scratch_bytes(ext_of(vol), abox)
    assert nbytes == 8 * n + 32 + 8 * (-(-w // 8) * -(-h // 8) * -(-d // 8)), (what, nbytes)
    d_scratch, h_scratch = T.guarded((nbytes // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_seeds, h_seeds = T.guarded(np.ascontiguousarray(seeds, np.uint32).view(np.int32), 0, FILL, "cuda")
    d_dist, h_dist = T.guarded(shape, 0, FILL, "cuda", dtype=np.int32)
    d_labels, h_labels = (d_seeds, h_seeds) if in_place else T.guarded(shape, 0, FILL, "cuda", dtype=np.int32)
    d_counts, h_counts = T.guarded((2,), 0, FILL, "cuda", dtype=np.int64)
    trace = []
    for call in range(max_calls):
        rc = ctx.geodesic_propagate_rc(d_vol.data_ptr(), ext_of(vol), abox, ISO, None if call else d_seeds.data_ptr(), steps, limit, rounds, call > 0,
                                       d_scratch.data_ptr(), d_dist.data_ptr() if want_dist else None, d_labels.data_ptr() if want_labels else None,
                                       d_counts.data_ptr(), st())
        assert rc == abi.VKV_OK, (what, call, rc, ctx.last_error())
        torch.cuda.synchronize()
        trace.append(int(d_counts[0].item()))
        assert trace[-1] in (0, 1), (what, trace)
        if trace[-1] == 1:
            break
    assert trace[-1] == 1, "%s: not settled after %d calls of %d rounds" % (what, max_calls, rounds)
    for name, handle in (("d_volume", h_vol), ("d_scratch", h_scratch), ("d_seeds", h_seeds), ("d_dist", h_dist), ("d_labels", h_labels), ("d_counts", h_counts)):
        bad = guard_damage(handle)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], handle.start, handle.stop - 1)
    assert np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    if not in_place:
        assert np.array_equal(d_seeds.cpu().numpy().view(np.uint32), np.asarray(seeds, np.uint32)), "%s: the seeds changed" % what
    for given, buf, name in ((want_dist, d_dist, "d_dist"), (want_labels or in_place, d_labels, "d_labels")):
        if not given:
            assert (buf.view(torch.uint8).cpu().numpy() == FILL).all(), "%s: %s was not given and was written" % (what, name)
    return (d_dist.cpu().numpy().view(np.uint32) if want_dist else None, d_labels.cpu().numpy().view(np.uint32) if want_labels else None,
            int(d_counts[1].item()), trace)


def check(ctx, vol, seeds, steps, limits=(None,), box=None, want=None, what="", **kw):
    """every limit against the unlimited reference cut at it; the reached count"""
    want_d, want_l = geodesic_sweeps_np(vol, ISO, seeds, steps, None, box) if want is None else want
    device_volume = upload(vol)
    for limit in limits:
        w = "%s, steps %s, limit %s" % (what, steps, limit)
        got_d, got_l, reached, trace = run(ctx, vol, seeds, steps, limit, box=box, device_volume=device_volume, what=w, **kw)
        cut_d, cut_l = cut(want_d, want_l, limit)
        same(got_d, cut_d, w + ": d_dist")
        same(got_l, cut_l, w + ": d_labels")
        assert reached == int((cut_d != NONE).sum()), (w, reached)
    return trace


def random_seeds(shape, seed, share=0.03, labels=5):
    rng = np.random.default_rng(seed)
    seeds = np.where(rng.random(shape) < share, rng.integers(1, labels + 1, size=shape), 0).astype(np.uint32)
    seeds.flat[int(rng.integers(0, seeds.size))] = 2        # at least one, wherever it lands
    return seeds


def cases_of(shape, seed):
    """(name, vol, seeds) of every content for one shape [d, h, w]"""
    out = []
    for axis in range(3):
        if shape[axis] % 2 == 1 and shape[axis] > 1:
            for first_small in (True, False):
                out.append(("mirrored %s %s" % ("zyx"[axis], first_small),) + mirrored_seeds(shape, axis, first_small))
    out.append(("checkerboard",) + checkerboard_seeds(shape, seed))
    out.append(("extreme labels",) + extreme_labels(shape))
    for k, density in enumerate((0.35, 0.6, 0.9)):
        out.append(("random %s" % density, contents("random %s" % density, shape, seed + k), random_seeds(shape, seed + 10 + k)))
    return out


# ---- every extent ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_content_step_table_and_limit(ctx, extent):
    w, h, d = extent
    for name, vol, seeds in cases_of((d, h, w), seed=w * 100 + h * 10 + d):
        for steps in TABLES:
            check(ctx, vol, seeds, steps, limits_of(steps), what="%s %s" % (name, extent), rounds=16)


@pytest.fixture(scope="module")
def several_hundred_tiles():
    """70 x 66 x 65: 9 x 9 x 9 tiles.  (name, vol, seeds, steps, the unlimited reference by whole-box sweeps)"""
    shape = (65, 66, 70)
    out = []
    for name, density, share, steps in (("random 0.35", 0.35, 0.002, CHAMFER), ("random 0.6", 0.6, 0.0005, SPACING_STEPS), ("random 0.9", 0.9, 0.0002, STEPS_6)):
        vol, seeds = contents(name, shape, seed=7), random_seeds(shape, 70, share)
        out.append((name, vol, seeds, steps, geodesic_sweeps_np(vol, ISO, seeds, steps)))
    return out


@pytest.mark.parametrize("k", [0, 1, 2], ids=["random_0.35", "random_0.6", "random_0.9"])
def test_several_hundred_tiles_against_the_whole_box_sweeps(ctx, several_hundred_tiles, k):
    name, vol, seeds, steps, want = several_hundred_tiles[k]
    assert int((want[1] != 0).sum()) > 20000        # a body that spans the box
    check(ctx, vol, seeds, steps, (None, 20, 100000), want=want, what="%s 70x66x65" % name, rounds=8)


def test_a_box_inside_a_larger_volume_does_not_see_its_surroundings(ctx):
    """the surroundings are inside voxels, and the guard bytes around the box-shaped d_seeds are non-zero: neither may leak in"""
    rng = np.random.default_rng(31)
    vol = np.full((20, 21, 40), 200, np.uint8)
    for box in [(5, 6, 7, 17, 9, 10), (0, 0, 0, 8, 8, 8), (23, 12, 10, 17, 9, 10), (3, 3, 3, 1, 1, 9), (1, 1, 1, 33, 17, 9)]:
        x0, y0, z0, w, h, d = box
        inner = contents("random 0.5", (d, h, w), seed=w)
        v = vol.copy()
        v[z0:z0 + d, y0:y0 + h, x0:x0 + w] = inner
        seeds = random_seeds((d, h, w), int(rng.integers(1000)))
        for steps in (CHAMFER, STEPS_6):
            want = geodesic_np(inner, ISO, seeds, steps)        # nothing beyond the box exists
            check(ctx, v, seeds, steps, (None, 20), box=box, want=want, what="box %s" % (box,))
            assert np.array_equal(np.ascontiguousarray(crop(v, box)), inner)


# ---- tile seams -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti", [False, True], ids=["diagonal", "anti-diagonal"])
def test_a_staircase_through_tile_corners(ctx, anti):
    vol, _ = staircase(35, anti)
    i = np.arange(35)
    on = (i, i, 34 - i if anti else i)
    seeds = np.zeros(vol.shape, np.uint32)
    seeds[34, 34, 0 if anti else 34] = 7        # in the LAST tile: the path runs against the order in which workgroups start
    for steps, rounds in ((CHAMFER, 2), (STEPS_26, 64), (STEPS_6, 2)):
        got_d, got_l, reached, trace = run(ctx, vol, seeds, steps, None, rounds=rounds, what="staircase %s" % (steps,))
        want_d, want_l = geodesic_np(vol, ISO, seeds, steps)
        same(got_d, want_d, "staircase: d_dist")
        same(got_l, want_l, "staircase: d_labels")
        if steps is STEPS_6:
            assert reached == 1 and trace == [1]        # no move exists: settled in the first call
        else:
            assert reached == 35 and np.array_equal(got_d[on], steps[6] * (34 - i))
            assert rounds != 2 or trace[0] == 0        # five tiles along the diagonal: two rounds do not get there


@pytest.mark.parametrize("scene", ["serpentine", "needle"])
def test_one_round_per_call_resumes_to_the_one_shot_answer(ctx, scene):
    if scene == "serpentine":
        vol, seeds = (np.ascontiguousarray(a[:, ::-1, ::-1]) for a in serpentine(40, 40, 3))        # the seed in the last tile: see the staircase
        steps = STEPS_6
    else:
        vol = np.full((1, 1, 200), 200, np.uint8)
        seeds = np.zeros((1, 1, 200), np.uint32)
        seeds[0, 0, 199] = 6
        steps = CHAMFER
    want_d, want_l = geodesic_np(vol, ISO, seeds, steps)
    got_d, got_l, reached, trace = run(ctx, vol, seeds, steps, None, rounds=1, max_calls=400, what=scene)
    assert trace[0] == 0 and trace[-1] == 1 and trace.count(1) == 1, trace        # the resume path ran
    # A key crosses a tile seam between rounds only, unless a racing halo load happens to see the neighbour's store of the same round, which
    # the seed in the last tile makes unlikely.  Without such luck the needle takes 25 rounds, one per tile, and one that finds nothing to
    # do; the serpentine 85 (100 row segments of a tile's width, 15 of its 19 turns inside one tile) and one.  A tile edge of 200 would
    # settle the needle in the first call; what is asked for here is a round per tile of the needle, and no more of the serpentine
    assert len(trace) >= 25, len(trace)
    same(got_d, want_d, scene + ": d_dist")
    same(got_l, want_l, scene + ": d_labels")
    one_d, one_l, one_reached, one_trace = run(ctx, vol, seeds, steps, None, rounds=1024, what=scene + " in one call")
    assert one_trace == [1] and one_reached == reached == int((vol >= 128).sum())
    same(one_d, got_d, scene + ": the one-shot d_dist")
    same(one_l, got_l, scene + ": the one-shot d_labels")


def test_costs_that_would_reach_2_to_the_32_minus_1_are_not_reached(ctx):
    vol = np.full((1, 1, 70000), 200, np.uint8)
    seeds = np.zeros((1, 1, 70000), np.uint32)
    seeds[0, 0, 0] = 0xfffffffe
    steps = (65535, 1, 1, 1, 1, 1, 1)
    got_d, got_l, reached, trace = run(ctx, vol, seeds, steps, None, rounds=1024, max_calls=12, what="70000 x 1 x 1")
    cost = 65535 * np.arange(70000, dtype=np.uint64)
    ok = cost < np.uint64(NONE)        # 65535 * 65537 = 2^32 - 1: the first that is not
    assert int(ok.sum()) == 65537 == reached and len(trace) >= 8
    same(got_d, np.where(ok, cost, NONE).astype(np.uint32).reshape(1, 1, -1), "d_dist")
    same(got_l, np.where(ok, 0xfffffffe, 0).astype(np.uint32).reshape(1, 1, -1), "d_labels")


# ---- arguments and state --------------------------------------------------------------------------------------------------------------------
def test_either_output_alone_in_place_seeds_on_outside_voxels_and_no_seed(ctx):
    shape = (10, 9, 17)
    vol = contents("random 0.6", shape, seed=3)
    seeds = random_seeds(shape, 4, share=0.05)
    seeds[vol < 128] = 9        # seed values on every outside voxel: ignored
    want_d, want_l = geodesic_np(vol, ISO, seeds, CHAMFER)
    for limit in (None, 7):
        cut_d, cut_l = cut(want_d, want_l, limit)
        got_d, got_l, reached, _ = run(ctx, vol, seeds, CHAMFER, limit, want_dist=False, what="d_dist NULL")
        assert got_d is None
        same(got_l, cut_l, "d_dist NULL: d_labels")
        got_d, got_l, reached2, _ = run(ctx, vol, seeds, CHAMFER, limit, want_labels=False, what="d_labels NULL")
        assert got_l is None and reached == reached2 == int((cut_d != NONE).sum())
        same(got_d, cut_d, "d_labels NULL: d_dist")
        got_d, got_l, _, _ = run(ctx, vol, seeds, CHAMFER, limit, in_place=True, rounds=2, what="in place")        # resumed calls write the labels again
        same(got_l, cut_l, "in place: d_labels")
        same(got_d, cut_d, "in place: d_dist")
    assert (want_l[vol < 128] == 0).all() and (want_d[vol < 128] == NONE).all()
    got_d, got_l, reached, trace = run(ctx, vol, np.zeros(shape, np.uint32), CHAMFER, None, rounds=1, what="no seed")
    assert reached == 0 and trace == [1] and (got_d == NONE).all() and (got_l == 0).all()
    got_d, got_l, reached, trace = run(ctx, vol, np.where(vol < 128, 5, 0).astype(np.uint32), CHAMFER, None, rounds=1, what="seeds outside only")
    assert reached == 0 and trace == [1] and (got_d == NONE).all() and (got_l == 0).all()


def test_surplus_rounds_change_nothing_and_two_runs_give_the_same_bytes(ctx):
    shape = (19, 21, 37)
    vol = contents("random 0.5", shape, seed=21)
    seeds = random_seeds(shape, 22)
    e = ext_of(vol)
    d_vol = torch.from_numpy(vol).cuda()
    d_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
    want_d, want_l = geodesic_np(vol, ISO, seeds, SPACING_STEPS)
    results = []
    d_scratch = torch.full((geodesic.scratch_bytes(e) // 8,), -1, dtype=torch.int64, device="cuda")
    for run_no in range(2):        # the second run starts from the first run's scratch
        d_dist = torch.full(shape, -1, dtype=torch.int32, device="cuda")
        d_labels = torch.full(shape, -1, dtype=torch.int32, device="cuda")
        d_counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        args = (SPACING_STEPS, None, 256)
        ctx.check(ctx.geodesic_propagate_rc(d_vol.data_ptr(), e, None, ISO, d_seeds.data_ptr(), *args, False, d_scratch.data_ptr(), d_dist.data_ptr(),
                                            d_labels.data_ptr(), d_counts.data_ptr(), st()))
        torch.cuda.synchronize()
        assert d_counts.tolist() == [1, int((want_l != 0).sum())]
        first = (d_dist.cpu().numpy().view(np.uint32), d_labels.cpu().numpy().view(np.uint32), d_scratch.cpu().numpy()[:vol.size].copy())
        for rounds in (1, 1024):        # a surplus of rounds after the fixed point
            ctx.check(ctx.geodesic_propagate_rc(d_vol.data_ptr(), e, None, ISO, None, SPACING_STEPS, None, rounds, True, d_scratch.data_ptr(), d_dist.data_ptr(),
                                                d_labels.data_ptr(), d_counts.data_ptr(), st()))
            torch.cuda.synchronize()
            assert d_counts.tolist() == [1, int((want_l != 0).sum())]
            same(d_dist.cpu().numpy().view(np.uint32), first[0], "after %d more rounds: d_dist" % rounds)
            same(d_labels.cpu().numpy().view(np.uint32), first[1], "after %d more rounds: d_labels" % rounds)
            assert np.array_equal(d_scratch.cpu().numpy()[:vol.size], first[2])        # the keys
        results.append(first)
    same(results[0][0], want_d, "d_dist")
    same(results[0][1], want_l, "d_labels")
    assert all(np.array_equal(a, b) for a, b in zip(results[0], results[1]))


def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((16384,), FILL, dtype=torch.uint8, device="cuda")        # [scratch 4096 | seeds 2048 | dist 2048 | labels 2048 | counts 2048 | spare]
    a = out.data_ptr()
    block = geodesic.scratch_bytes(e)
    assert a % 8 == 0 and block == 8 * 240 + 32 + 8 * 2 <= 4096
    scratch, seeds, dist, labels, counts, v = a, a + 4096, a + 6144, a + 8192, a + 10240, vol.data_ptr()
    bad, unsupported, inf, nan = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED, float("inf"), float("nan")
    S = CHAMFER

    def rc(volume=v, extent=e, box=None, iso=0.5, d_seeds=seeds, steps=S, limit=5, rounds=3, resume=0, d_scratch=scratch, d_dist=dist, d_labels=labels,
           d_counts=counts):
        return ctx.geodesic_propagate_rc(volume, extent, box, iso, d_seeds, steps, limit, rounds, resume, d_scratch, d_dist, d_labels, d_counts, st())

    for null in ("volume", "d_scratch", "d_counts", "steps", "d_seeds"):
        assert rc(**{null: None}) == bad and "null" in ctx.last_error(), null
    assert rc(d_dist=None, d_labels=None) == bad and "neither" in ctx.last_error()
    assert rc(extent=abi.Extent3D(w, 0, d)) == bad
    for box in (abi.Box(0, 0, 0, 13, 2, 2), abi.Box(11, 4, 3, 1, 2, 1), abi.Box(1, 1, 1, 2, 0, 2)):
        assert rc(box=box) == bad and "box" in ctx.last_error()
    for iso in (inf, -inf, nan):
        assert rc(iso=iso) == bad and "iso" in ctx.last_error()
    assert rc(limit=0) == bad and "limit" in ctx.last_error()
    for rounds in (0, 1025, 0xffffffff):
        assert rc(rounds=rounds) == bad and "rounds" in ctx.last_error()
    for resume in (2, -1, 256):
        assert rc(resume=resume) == bad and "resume" in ctx.last_error()
        assert rc(resume=resume, d_seeds=None) == bad
    assert rc(steps=(0,) * 7) == bad and "step" in ctx.last_error()
    for m in range(7):
        assert rc(steps=tuple(65536 if k == m else 1 for k in range(7))) == bad and "step" in ctx.last_error()
    for name, off in (("d_seeds", 2), ("d_dist", 2), ("d_labels", 1), ("d_counts", 4), ("d_scratch", 4)):
        assert rc(**{name: {"d_seeds": seeds, "d_dist": dist, "d_labels": labels, "d_counts": counts, "d_scratch": scratch}[name] + off}) == bad \
            and "aligned" in ctx.last_error(), name
    # the overlaps: 240 voxels are 960 bytes; the block is 1968
    for other in (seeds + 4, seeds + 956, seeds - 956):
        assert rc(d_labels=other) == bad and "overlap" in ctx.last_error()
    for other in (seeds, seeds + 4, seeds + 956, seeds - 956, labels, labels + 956, labels - 956):
        assert rc(d_dist=other) == bad and "overlap" in ctx.last_error()
    for name in ("d_seeds", "d_dist", "d_labels"):
        for other in (scratch, scratch + 8, scratch + block - 4, scratch - 956):
            assert rc(**{name: other}) == bad and "overlap" in ctx.last_error(), (name, other - scratch)
    assert rc(d_dist=seeds, d_labels=None) == bad and rc(d_seeds=dist, d_labels=None) == bad
    assert rc(extent=abi.Extent3D(65536, 65536, 1)) == unsupported        # 2^32 voxels: one too many
    assert rc(extent=abi.Extent3D(2048, 2048, 2048), box=abi.Box(0, 0, 0, 2048, 2048, 1024)) == unsupported
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # the accepted neighbours write: arrays right behind one another, d_labels == d_seeds, a resumed call without seeds
    out[4096:6144] = 0
    assert rc(d_dist=seeds + 960, d_labels=seeds, d_scratch=scratch, limit=None, rounds=1024) == abi.VKV_OK
    assert rc(d_seeds=None, resume=1, d_dist=seeds + 960, d_labels=seeds, limit=None, rounds=1) == abi.VKV_OK
    torch.cuda.synchronize()
    assert out[10240:10256].view(torch.int64).tolist() == [1, 0] and bool((out[4096:4096 + 960] == 0).all())        # no seed: nothing reached
    assert bool((out[4096 + 960:4096 + 1920].view(torch.int32) == -1).all()) and bool((out[4096 + 1920:6144] == 0).all()) and bool((out[6144:10240] == FILL).all())


# ---- capture -----------------------------------------------------------------------------------------------------------------------------------
def test_a_fixed_round_call_captured_into_a_graph_replays_the_direct_calls_bytes(ctx):
    shape = (17, 9, 131)
    vol = contents("random 0.6", shape, seed=13)
    seeds = random_seeds(shape, 14)
    e = ext_of(vol)
    d_vol = torch.from_numpy(vol).cuda()
    d_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
    d_scratch = torch.empty((geodesic.scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    d_dist = torch.empty(shape, dtype=torch.int32, device="cuda")
    d_labels = torch.empty(shape, dtype=torch.int32, device="cuda")
    d_counts = torch.empty((2,), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def call():
        ctx.check(ctx.geodesic_propagate_rc(d_vol.data_ptr(), e, None, ISO, d_seeds.data_ptr(), CHAMFER, 60, 48, False, d_scratch.data_ptr(), d_dist.data_ptr(),
                                            d_labels.data_ptr(), d_counts.data_ptr(), s.cuda_stream))

    torch.cuda.synchronize()
    with torch.cuda.stream(s):        # one direct call on the capture stream
        call()
    torch.cuda.synchronize()
    assert int(d_counts[0].item()) == 1
    direct = (d_dist.cpu().numpy().view(np.uint32), d_labels.cpu().numpy().view(np.uint32), d_counts.tolist())
    want_d, want_l = geodesic_np(vol, ISO, seeds, CHAMFER, 60)
    same(direct[0], want_d, "direct: d_dist")
    same(direct[1], want_l, "direct: d_labels")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    torch.cuda.synchronize()
    for replay in range(2):        # the outputs and the state overwritten, then the graph replayed
        for t in (d_dist, d_labels, d_counts, d_scratch):
            t.view(torch.uint8).fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        same(d_dist.cpu().numpy().view(np.uint32), direct[0], "replay %d: d_dist" % replay)
        same(d_labels.cpu().numpy().view(np.uint32), direct[1], "replay %d: d_labels" % replay)
        assert d_counts.tolist() == direct[2] == [1, int((want_l != 0).sum())]


# ---- Volume.geodesic_propagate / grow_from_points / split_bodies --------------------------------------------------------------------------------
def test_volume_geodesic_propagate_and_grow_from_points_against_the_numpy_statements(ctx):
    vol = contents("random 0.5", (31, 26, 37), seed=4)
    v = make_volume(ctx, vol, block=2, packed=False)
    seeds = random_seeds(vol.shape, 8, share=0.001)
    d_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
    for steps, limit in ((None, None), (STEPS_6, 12), (BIG_STEPS, None)):
        labels, dist, counts = v.geodesic_propagate(d_seeds, ISO, steps=steps, limit=limit)
        want_d, want_l = geodesic_np(vol, ISO, seeds, steps or CHAMFER, limit)
        assert labels.dtype == dist.dtype == torch.uint32 and counts.tolist() == [1, int((want_l != 0).sum())]
        same(dist.cpu().numpy(), want_d, "Volume.geodesic_propagate(%s, %s): dist" % (steps, limit))
        same(labels.cpu().numpy(), want_l, "Volume.geodesic_propagate(%s, %s): labels" % (steps, limit))
    labels, dist, counts = v.geodesic_propagate(d_seeds, ISO, rounds=1, distance=False)        # one call, whatever it reaches
    assert dist is None and counts.tolist()[0] in (0, 1)
    box = ((3, 2, 5), (20, 17, 9))
    b = (3, 2, 5, 20, 17, 9)
    box_seeds = np.ascontiguousarray(crop(seeds, b))
    labels, dist, counts = v.geodesic_propagate(torch.from_numpy(box_seeds.view(np.int32)).cuda(), ISO, box=box)
    want_d, want_l = geodesic_np(vol, ISO, box_seeds, CHAMFER, None, b)
    same(dist.cpu().numpy(), want_d, "box: dist")
    same(labels.cpu().numpy(), want_l, "box: labels")
    # click to select: points i carry i + 1; the second click lies on an outside voxel and seeds nothing
    inside = np.argwhere(vol >= 128)
    outside = np.argwhere(vol < 128)
    points = [tuple(int(c) for c in inside[5][::-1]), tuple(int(c) for c in outside[7][::-1]), tuple(int(c) for c in inside[-3][::-1])]
    clicks = np.zeros(vol.shape, np.uint32)
    for k, (x, y, z) in enumerate(points):
        clicks[z, y, x] = k + 1
    for limit in (None, 25):
        labels, dist, counts = v.grow_from_points(points, ISO, limit=limit)
        want_d, want_l = geodesic_np(vol, ISO, clicks, CHAMFER, limit)
        assert set(np.unique(want_l).tolist()) <= {0, 1, 3} and counts.tolist() == [1, int((want_l != 0).sum())]
        same(dist.cpu().numpy(), want_d, "grow_from_points(limit=%s): dist" % limit)
        same(labels.cpu().numpy(), want_l, "grow_from_points(limit=%s): labels" % limit)
    same(v.volume.cpu().numpy(), vol, "the volume itself")


def test_volume_split_bodies_geodesic_leaves_the_fragment_across_the_gap_unlabelled(ctx):
    from scipy import ndimage
    vol, bridge, ball = gap_scene()
    v = make_volume(ctx, vol, block=2, packed=False)
    inside = vol >= 128
    for r2, connectivity, weights in ((4, 6, None), (2, 26, None), (16, 6, (2, 2, 2))):
        labels, counts = v.split_bodies(ISO, radius2=r2, connectivity=connectivity, weights=weights, metric="geodesic")
        want, k = split_bodies_geodesic_np(vol, ISO, r2, connectivity, weights)
        what = "Volume.split_bodies(radius2=%d, connectivity=%d, weights=%s, metric='geodesic')" % (r2, connectivity, weights)
        assert labels.dtype == torch.uint32 and int(counts[0].item()) == k == 2, what
        same(labels.cpu().numpy(), want, what)
        assert (want[ball] == 0).all() and np.array_equal(want != 0, inside & ~ball), what
        sizes = v.component_stats(labels, counts, values=False).voxels.cpu().numpy()
        assert len(sizes) == 2 and int(sizes.sum()) == int(inside.sum()) - int(ball.sum()) and sizes[0] == sizes[1], what        # two bodies: the mask less the ball
    # the default is what it was: the Euclidean split, which labels the fragment
    for kw in ({}, {"metric": "euclidean"}):
        labels, counts = v.split_bodies(ISO, radius2=4, **kw)
        want, k = split_bodies_np(vol, ISO, 4)
        same(labels.cpu().numpy(), want, "Volume.split_bodies, the default")
        assert int(counts[0].item()) == k == 2 and (want[ball] == 1).all()
    plain, _ = bridge_scene()
    p = make_volume(ctx, plain, block=2, packed=False)
    for r2, connectivity, weights in ((2, 6, None), (4, 6, None), (2, 26, None), (4, 6, (1, 1, 2))):        # the cases of tests/test_gpu_nearest.py
        labels, counts = p.split_bodies(ISO, radius2=r2, connectivity=connectivity, weights=weights)
        want, k = split_bodies_np(plain, ISO, r2, connectivity, weights)
        same(labels.cpu().numpy(), want, "Volume.split_bodies(radius2=%d, connectivity=%d, weights=%s) as before" % (r2, connectivity, weights))
        assert int(counts[0].item()) == k
    same(v.volume.cpu().numpy(), vol, "the volume itself")
    assert ndimage.label(inside, structure=np.ones((3, 3, 3)))[1] == 2
