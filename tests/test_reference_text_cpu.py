"""The oracle against the reference's OWN shader text.  oracle/_ref/libvkv_ref.so is gradient_map.comp, occupancy_map.comp, distance_map.comp,
distance_map_anisotropic.comp and volume_render.frag themselves, compiled as C++ for the CPU (oracle/glsl_host/: a GLSL shim, an anchored
preprocessing recipe and a harness - none of it restates a shader).  Every other pin of oracle/vkv_oracle.c was written by this project's authors
from their reading of those files; a shared misreading passes all of them and fails here.

The library is built where a checkout of the reference is present (`make -C oracle ref`, __graft_entry__.build()); without it these tests skip.

  maps      gradient map, occupancy map (precomputed / on-the-fly gradient, texture transfer function, blocks 2..6), isotropic distance map, all
            eight anisotropic maps: every byte equal.
  frag      "pinned" shim arithmetic: the three counters of every pixel equal, colour within COLOR_TOL, depth within
            DEPTH_TOL.  "plain" arithmetic: counters equal tests/golden/frag_literal.py in its "plain" mode at EVERY covered pixel (the literal
            is then a proven transliteration), and differ from the oracle within the caps tests/test_frag_literal_cpu.py states.
  depth     DEPTH_ATTACHMENT: discard decisions and counters equal outside the pixels whose wall lies within 4 ulp of the front face.
  fixture   tests/golden/reference_v1.npz is what a fresh run gives."""
import numpy as np
import pytest

from oracle import vkv_oracle as O
from oracle import vkv_ref as R
from tests import helpers as T
from tests.golden import comp_literal as CL
from tests.golden import make_reference_vectors as G
from tests.test_gpu_parity import COLOR_TOL, DEPTH_TOL
from vkvolume_amd import abi

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libvkv_ref.so is not built: no checkout of the reference at build time")

NO_GRADIENT_TF = dict(intensity_min=0.1, gradient_min=0.0, gradient_max=0.0)  # use_gradient = 0


def volumes():
    """name -> (volume [D,H,W], transfer function options).  Extents that are no multiple of any block, dimensions below the block size; `empty`
    gives an all-empty map (alpha 0 everywhere), `solid` an all-occupied one (no gradient term, every voxel above the threshold)."""
    return {
        "shells36x30x26": (O.synth_volume((36, 30, 26), 1, 0xC0FFEE02), T.APP_TF),
        "random13x7x5": (T.random_volume((13, 7, 5), 5, 0.7), T.APP_TF),
        "random10x3x3": (T.random_volume((10, 3, 3), 6, 0.9), T.APP_TF),
        "shells4x5x6": (O.synth_volume((4, 5, 6), 1, 7), T.APP_TF),
        "sparse33x17x9": (T.random_volume((33, 17, 9), 8, 0.995), NO_GRADIENT_TF),
        "empty11x6x7": (np.zeros((7, 6, 11), np.uint8), T.APP_TF),
        "solid9x8x5": (np.full((5, 8, 9), 200, np.uint8), NO_GRADIENT_TF),
    }


VOLUME_NAMES = list(volumes())


def random_texture(seed):
    """a transfer-function texture that is no product of two ramps: random RGBA with alpha zero in random rows and columns"""
    rng = np.random.default_rng(seed)
    tex = rng.integers(1, 256, (256, 256, 4), dtype=np.uint8)
    tex[rng.random(256) < 0.5, :, 3] = 0
    tex[:, rng.random(256) < 0.5, 3] = 0
    return tex


@pytest.mark.parametrize("name", VOLUME_NAMES)
def test_gradient_map(name):
    vol, tfo = volumes()[name]
    for options in (abi.VolumeOptions(**tfo), abi.VolumeOptions(**T.APP_TF), abi.VolumeOptions(**NO_GRADIENT_TF)):
        tf = O.transfer_function_uniform(options)
        for modifier in (1.0, 2.5, 0.37):
            tf.grad_magnitude_modifier = modifier
            assert np.array_equal(O.gradient_map(vol, tf), R.gradient_map(vol, tf)), "use_gradient %d modifier %g" % (tf.use_gradient, modifier)


@pytest.mark.parametrize("name", VOLUME_NAMES)
def test_occupancy_and_distance_maps(name):
    vol, tfo = volumes()[name]
    seen = set()
    for on_the_fly in (False, True):
        scene = T.OracleScene(vol, abi.VolumeOptions(use_precomputed_gradient=not on_the_fly, **tfo), 4)
        for tex in (scene.tex, random_texture(len(name))):
            for block in (2, 3, 4, 5, 6):
                what = "%s gradient, block %d" % ("on-the-fly" if on_the_fly else "precomputed", block)
                occ = O.occupancy_map(vol, scene.grad, tex, scene.tf, block)
                assert np.array_equal(occ, R.occupancy_map(vol, scene.grad, tex, scene.tf, block)), "occupancy, " + what
                seen.add("empty" if (occ == 255).all() else ("occupied" if (occ == 0).all() else "mixed"))
                assert np.array_equal(O.distance_map(occ), R.distance_map(occ)), "distance map, " + what
                got, expect = R.distance_map_anisotropic(occ), O.distance_map_anisotropic(occ)
                for k in range(8):
                    assert np.array_equal(expect[k], got[k]), "anisotropic map %d, %s" % (k, what)
    # the premise of the case: what kind of map it was chosen for
    assert seen >= {"empty11x6x7": {"empty"}, "solid9x8x5": {"occupied"}}.get(name, {"mixed"}), seen


def test_occupancy_map_extent_that_is_not_the_quotient():
    """a map extent that is not ceil(extent / block): the block follows from it (src/compute_distance_map.cpp:110-113) and the last cells hold no
    voxel (the shader clips a cell at the volume's edge, occupancy_map.comp:52-53)"""
    vol = T.random_volume((16, 16, 16), 9, 0.9)
    scene = T.OracleScene(vol, abi.VolumeOptions(**T.APP_TF), 4)
    me = abi.Extent3D(7, 7, 7)
    expect = O.occupancy_map(vol, scene.grad, scene.tex, scene.tf, 0, map_extent_override=me)
    assert np.array_equal(expect, R.occupancy_map(vol, scene.grad, scene.tex, scene.tf, 0, map_extent_override=me))
    assert (expect[6] == 255).all() and 0 < (expect == 0).mean() < 1


@pytest.mark.parametrize("shape_dhw", [(9, 10, 13), (2, 300, 3), (300, 2, 3), (3, 2, 300), (1, 1, 1), (5, 70, 3)])
def test_distance_transforms_on_occupancy_maps_of_their_own(shape_dhw):
    """Maps that no small volume gives: axes beyond 255 cells (the transforms saturate there: one occupied cell at the first or at the last corner, so
    that distances up to 254 and the 255 behind them occur along the long axis in either direction), a single cell, and ARBITRARY bytes (both shaders
    are defined for any input).  Also the harness's restated dispatch schedule against comp_literal.py's, on the smallest map."""
    rng = np.random.default_rng(sum(shape_dhw))
    first, last = np.full(shape_dhw, 255, np.uint8), np.full(shape_dhw, 255, np.uint8)
    first[0, 0, 0] = 0
    last[-1, -1, -1] = 0
    raw = rng.integers(0, 256, size=shape_dhw, dtype=np.uint8)
    raw[rng.random(shape_dhw) < 0.7] = 255
    for m in (first, last, raw):
        assert np.array_equal(O.distance_map(m), R.distance_map(m))
        got, expect = R.distance_map_anisotropic(m), O.distance_map_anisotropic(m)
        for k in range(8):
            assert np.array_equal(expect[k], got[k]), "octant %d" % k
    if max(shape_dhw) > 255:
        for m in (first, last):
            assert 254 in O.distance_map_anisotropic(m) and 254 in O.distance_map(m)
    if raw.size <= 2000:
        lit = CL.distance_map_anisotropic(raw)
        for k in range(8):
            assert np.array_equal(lit[k], R.distance_map_anisotropic(raw)[k]), "schedule: octant %d" % k
        assert np.array_equal(CL.distance_map(raw), R.distance_map(raw))


# ---- fragment shader ----------------------------------------------------------------------------------------------------------------
IMAGE = (48, 48)
_SCENES = {}


def scene_for(sf, on_the_fly=False):
    key = (sf, on_the_fly)
    if key not in _SCENES:
        opt = abi.VolumeOptions(sampling_factor=sf, use_precomputed_gradient=not on_the_fly, **T.APP_TF)
        _SCENES[key] = T.OracleScene(G.volume(), opt, 4, voxel_size=(0.0003, 0.0003, 0.0007), axis_angle=(1, 0, 0, 90))
    return _SCENES[key]


def oracle_and_entry(scene, view, proj, size, clip_distance=1.0, test=abi.TEST_NONE, **options):
    """the frame's parameter block, and the one that makes the oracle output its ray entries (rgb = ray_entry, a = 1 where there is a fragment)"""
    p = scene.params(view, proj, size, abi.RenderOptions(clip_distance=clip_distance, test=test, **options))
    pe = scene.params(view, proj, size, abi.RenderOptions(clip_distance=clip_distance, test=abi.TEST_RAY_ENTRY, **options))
    return p, pe


def text_frag(scene, p, entry, **kw):
    mode = p.options.skipping_type
    return R.frag(p, entry, scene.vol, scene.grad, scene.tex, None if mode == abi.SKIP_NONE else scene.maps(mode), **kw)


def assert_frame_equal(r, ref, what):
    bad = np.argwhere((r.counts != ref.counts).any(-1))
    assert len(bad) == 0, "%s: counters differ in %d pixels, first %r: text %r oracle %r" % (
        what, len(bad), bad[0].tolist(), r.counts[tuple(bad[0])].tolist(), ref.counts[tuple(bad[0])].tolist())
    dc, dd = float(np.abs(r.color - ref.color).max()), float(np.abs(r.depth - ref.depth).max())
    print("%s: colour differs by %g, depth by %g" % (what, dc, dd))
    assert dc <= COLOR_TOL, "%s: colour differs by %g" % (what, dc)
    assert dd <= DEPTH_TOL, "%s: depth differs by %g" % (what, dd)


@pytest.mark.parametrize("sf", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("ert", [True, False])
@pytest.mark.parametrize("mode", [abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_frag_pinned(mode, ert, sf):
    scene = scene_for(sf)
    view, proj = T.orbit(33.0 + 40.0 * mode, image_size=IMAGE)
    p, pe = oracle_and_entry(scene, view, proj, IMAGE, skipping_type=mode, early_ray_termination=ert)
    ref, entry = scene.render(p), scene.render(pe).color
    assert ref.counts[..., 0].sum() > 1000 and (mode == abi.SKIP_NONE or ref.counts[..., 1].sum() > 100)
    r = text_frag(scene, p, entry)
    assert np.array_equal(r.fragment, entry[..., 3] > 0)
    assert_frame_equal(r, ref, "mode %d ert %d sf %g" % (mode, ert, sf))


@pytest.mark.parametrize("mode", [abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_frag_pinned_on_the_fly_gradient(mode):
    """the #ifndef PRECOMPUTED_GRADIENT branch of get_gradient (frag:92-97)"""
    scene = scene_for(1.0, on_the_fly=True)
    view, proj = T.orbit(200.0 + 25.0 * mode, image_size=IMAGE)
    p, pe = oracle_and_entry(scene, view, proj, IMAGE, skipping_type=mode)
    ref = scene.render(p)
    assert ref.counts[..., 0].sum() > 1000
    assert_frame_equal(text_frag(scene, p, scene.render(pe).color), ref, "on-the-fly gradient, mode %d" % mode)


@pytest.mark.parametrize("test,show", [(abi.TEST_RAY_ENTRY, R.SHOW_RAY_ENTRY), (abi.TEST_RAY_EXIT, R.SHOW_RAY_EXIT)])
def test_frag_show_ray_entry_and_exit(test, show):
    """the SHOW_RAY_ENTRY / SHOW_RAY_EXIT outputs (frag:168-173): ray_caster_get_back and the interpolant itself"""
    scene = scene_for(1.0)
    for az in (33.0, 200.0):
        view, proj = T.orbit(az, image_size=IMAGE)
        p, pe = oracle_and_entry(scene, view, proj, IMAGE, skipping_type=abi.SKIP_DISTANCE, test=test)
        ref, entry = scene.render(p), scene.render(pe).color
        r = text_frag(scene, p, entry, show=show)
        assert (r.counts == 0).all() and (entry[..., 3] > 0).sum() > 400
        assert np.array_equal(r.color, ref.color)  # coordinates: the same bits


@pytest.mark.parametrize("mode", [abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_frag_pinned_axis_parallel_view(mode):
    """A camera on an axis of the box looking along it, image of odd size: the rays of the centre column and row have direction components
    that are exactly zero, step_dist_texel_inv is infinite there and 0 * inf a NaN (frag:239, 242; DESIGN.md section 3: that axis never
    limits the skip).  Inside the box behind the clipping plane as well."""
    scene = scene_for(1.0)
    size = (47, 47)
    for radius, clip in ((150.0, 1.0), (20.0, 5.0)):
        view, proj = T.orbit(0.0, elevation=0.0, radius=radius, image_size=size)
        p, pe = oracle_and_entry(scene, view, proj, size, skipping_type=mode, clip_distance=clip)
        ref, entry = scene.render(p), scene.render(pe).color
        cam = np.array(list(p.ray_cast.camera_pos_tex)[:3], np.float32)
        zero = ((entry[..., :3] - cam) == 0) & (entry[..., 3:] > 0)
        if radius == 150.0:
            assert zero.any(), "no ray of this view has a direction component that is exactly zero"
            assert ref.counts[..., 1][zero.any(-1)].sum() > 0, "no axis-parallel ray probes the map"
        assert_frame_equal(text_frag(scene, p, entry), ref, "axis-parallel, mode %d radius %g" % (mode, radius))


@pytest.mark.parametrize("sf", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("ert", [True, False])
@pytest.mark.parametrize("mode", [abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_frag_plain_equals_the_literal(mode, ert, sf):
    """The frames of tests/test_frag_literal_cpu.py (16 x 16; the literal is pure Python).  Plain arithmetic on both sides: the compiled text and
    the numpy transliteration must count the same at EVERY covered pixel.  Against the oracle (pinned arithmetic) the caps of that test apply:
    differing pixels <= max(2, 8 % of the covered ones), 20 % with block skipping - and every differing pixel is one where the text in pinned
    mode agrees with the oracle."""
    from tests.test_frag_literal_cpu import frame
    scene, p, ref, entry, literal_plain = frame(mode, ert, sf)
    covered = entry[..., 3] > 0
    plain = text_frag(scene, p, entry, mode=R.PLAIN)
    bad = np.argwhere((plain.counts != literal_plain).any(-1) & covered)
    assert len(bad) == 0, "plain text differs from the plain literal at %r: text %r literal %r" % (
        bad[:5].tolist(), [plain.counts[y, x].tolist() for y, x in bad[:5]], [literal_plain[y, x].tolist() for y, x in bad[:5]])
    differs = (plain.counts != ref.counts).any(-1)
    limit = 0.20 if mode == abi.SKIP_BLOCK else 0.08
    assert int(differs.sum()) <= max(2, limit * int(covered.sum())), "%d of %d pixels differ" % (int(differs.sum()), int(covered.sum()))
    pinned = text_frag(scene, p, entry)
    assert np.array_equal(pinned.counts[differs], ref.counts[differs])


# ---- DEPTH_ATTACHMENT ---------------------------------------------------------------------------------------------------------------
WALLS = [0.1 / 90.0, 0.1 / 110.0, 0.1 / 150.0, 0.5, 1e-6]  # reverse-Z depths: before, inside and behind the box, at the near plane, far away


def scene_depth(covered, seed):
    """the walls of test_depth_attachment_and_blend_fuzz - whole columns at one reverse-Z depth, 'far' (0) elsewhere - placed over the box's image so
    that every frame has a wall before the box (its fragments are discarded), one inside it (its rays end early), one more of the seed's choice
    and columns without a wall"""
    rng = np.random.default_rng(77000 + seed)
    in_depth = np.zeros(covered.shape, np.float32)
    columns = np.flatnonzero(covered.any(0))
    band = (int(columns[-1]) - int(columns[0]) + 1) // 4
    depths = rng.permutation([float(rng.choice([0.5, 0.1 / 90.0])), 0.1 / 150.0, float(rng.choice(WALLS))])
    for k, depth in enumerate(depths):
        x0 = int(columns[0]) + k * band + int(rng.integers(0, band // 2 + 1))
        in_depth[:, x0:x0 + int(rng.integers(band // 2, band + 1))] = depth
    return in_depth


def front_depth(p, entry):
    """frag:127 with `position` in the pinned form: three fma chains (each float32 fma from an exact double product and one double sum)"""
    def mat_vec(m, v):
        m = np.array(list(m), np.float32).reshape(4, 4).astype(np.float64)  # column-major: m[c] is column c
        r = np.float32(m[0] * v[..., 0:1])
        for c in (1, 2, 3):
            r = np.float32(m[c] * v[..., c:c + 1].astype(np.float64) + r.astype(np.float64))
        return r
    v = np.concatenate([np.float32(entry[..., :3] - np.float32(0.5)), np.ones_like(entry[..., :1])], -1).astype(np.float32)
    pos = mat_vec(p.camera.camera_proj, mat_vec(p.camera.camera_view, mat_vec(p.camera.model, v)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(pos[..., 2] / pos[..., 3])


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("mode", [abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_frag_depth_attachment(mode, seed):
    """frag:122-165: a fragment whose front face lies behind the scene depth is discarded, a ray ends where it meets the scene.  Discard
    decisions, counters, colour and depth against the oracle.  Only pixels whose wall lies within 4 ulp of the front-face depth are left out
    (there the comparison of :129 hangs on a rounding of `position`, which the rasteriser, not the shader, computes): at most 1 % of the
    covered pixels - a condition on the walls chosen here, asserted."""
    scene = scene_for(1.0)
    view, proj = T.orbit(33.0 + 40.0 * mode + 90.0 * seed, image_size=IMAGE)
    p, pe = oracle_and_entry(scene, view, proj, IMAGE, skipping_type=mode, depth_attachment=True)
    plain_entry = scene.params(view, proj, IMAGE, abi.RenderOptions(skipping_type=mode, clip_distance=1.0, test=abi.TEST_RAY_ENTRY))
    entry = scene.render(plain_entry).color  # every covered pixel, before the depth test
    covered = entry[..., 3] > 0
    in_depth = scene_depth(covered, seed + 2 * mode)
    ref = scene.render(p, in_depth=in_depth)
    ref_fragment = scene.render(pe, in_depth=in_depth).color[..., 3] > 0  # the oracle's discard decisions
    front = front_depth(p, entry)
    ulp = np.spacing(np.maximum(np.abs(front), np.abs(in_depth)).astype(np.float32))
    near_tie = covered & (np.abs(front.astype(np.float64) - in_depth) <= 4.0 * ulp)
    assert near_tie.sum() <= 0.01 * covered.sum(), "%d of %d pixels sit on the depth test" % (near_tie.sum(), covered.sum())
    keep = covered & ~near_tie
    discarded = keep & ~ref_fragment
    assert discarded.sum() > 20 and (keep & ref_fragment).sum() > 100, "the walls hide nothing, or everything"
    assert (ref.counts[..., 0][keep & (in_depth > 0)] > 0).any(), "no ray ends at a wall inside the box"
    r = text_frag(scene, p, entry, in_depth=in_depth)
    assert np.array_equal(r.fragment[keep], ref_fragment[keep]), "discard decisions differ"
    assert np.array_equal(r.counts[keep], ref.counts[keep]), "counters differ in %d pixels" % int((r.counts != ref.counts).any(-1)[keep].sum())
    assert float(np.abs(r.color - ref.color)[keep].max()) <= COLOR_TOL
    both = keep & ref_fragment
    assert float(np.abs(r.depth - ref.depth)[both].max()) <= DEPTH_TOL


# ---- fixture --------------------------------------------------------------------------------------------------------------------------
def test_committed_reference_vectors_are_a_fresh_run():
    gold = np.load(G.PATH)
    fresh = G.compute()
    assert sorted(gold.files) == sorted(fresh)
    for key in gold.files:
        assert gold[key].dtype == fresh[key].dtype and np.array_equal(gold[key], fresh[key]), key
