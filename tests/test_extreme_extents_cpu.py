"""Ray-march cases at needle, slab and one-voxel extents, and what the oracle alone says about them (no GPU, no HIP library).

The case table below is shared with tests/test_gpu_extreme_extents.py, which renders every case on the device against the oracle.  This file
asserts the premises that keep that comparison from passing on an empty frame - every case puts samples (and, with skipping, map probes) on a
good part of the image and has visible pixels - and, by arithmetic on the table, that the needles stand on both sides of every extent at which
the integrator's address-table machinery changes what it does.

The constants of that arithmetic, quoted from vkvolume_amd/csrc/raymarch_core.hpp (a change there must show up here as a failed premise, not move
the cases off their boundaries unnoticed):
    kFullLutWord  = 1028      words of RmLds in front of the per-voxel-index tables X[W + 2] | Y[H + 2] | Z[D + 2]
    full_lut_bytes(W, H, D)   = (W + 2 + H + 2 + D + 2) * 4
    kFullLdsLimit = 17920     bytes (= VkvTuning.full_table_lds_limit by default, host_arith.cpp); choose_lean (raymarch.hip) takes the per-voxel
                              tables while kFullLutWord * 4 + full_lut_bytes <= the limit, the two-level tables above
    full_lut_issue            copies the tables in 16-byte pieces, nvec = ceil((W + H + D + 6) / 4), one piece per thread and round of a 256-thread
                              workgroup, kFullCopyRounds = 4 unrolled rounds
Which table kind a launch took is INFERRED from this rule: the ABI has no accessor for it."""
import os
import re
import time

import numpy as np
import pytest

from oracle import vkv_oracle as O
from tests import helpers as T
from vkvolume_amd import abi

SIZE = (64, 48)
RADIUS = 150.0
SKIPS = (abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE)
NO_GRADIENT_TF = dict(intensity_min=0.1, gradient_min=0.0, gradient_max=0.0)
OBLIQUE = (33.0, 20.0)

# ---- the launcher's rule, restated (see the module docstring) ------------------------------------------------------------------------
FULL_LUT_WORD, FULL_LDS_LIMIT, PIECE_BYTES, WORKGROUP, COPY_ROUNDS = 1028, 17920, 16, 256, 4


def copy_pieces(whd):
    return -(-(sum(whd) + 6) * 4 // PIECE_BYTES)


def copy_rounds(whd):
    """rounds of the workgroup's table copy that have a piece to store"""
    return -(-copy_pieces(whd) // WORKGROUP)


def takes_per_voxel_tables(whd):
    return FULL_LUT_WORD * 4 + (sum(whd) + 6) * 4 <= FULL_LDS_LIMIT


LDS_BASE, RMLDS_BYTES = 16, (256 + 2048 + 256) * 4        # kLdsBase; sizeof(RmLds): float alpha[256], uint32_t bits[2048], float unorm[256]


def lut_words(whd):
    """length of the two-level tables (build_addr_tables, addr_tables.hpp): 96 in-brick words, one macro-brick term per 32 padded indices of x and
    y (z starts on an even word) and a 64-bit one of z"""
    nmx, nmy, nmz = ((e + 1) // 32 + 1 for e in whd)
    return ((96 + nmx + nmy + 1) & ~1) + 2 * nmz


def lean_choice(whd):
    """(table kind, dynamic LDS bytes, lut_words) of a packed volume under the default tuning: choose_lean and lean_lds_bytes restated.
    launch_render_batch keeps one kernel for a batch whose frames agree in all three and takes the register fallback otherwise."""
    two_level = LDS_BASE + RMLDS_BYTES + lut_words(whd) * 4
    if not takes_per_voxel_tables(whd):
        return 1, two_level, lut_words(whd)
    full_end = LDS_BASE + FULL_LUT_WORD * 4 + (((sum(whd) + 6) * 4 + 15) & ~15)
    return 2, max(two_level, full_end), lut_words(whd)


def batch_shares_a_kernel(extents):
    return len({lean_choice(e) for e in extents}) == 1


# W + H + D on the two sides of each boundary: rounds 1, 2, 3 of the copy start at the upper value; above the last pair the two-level tables
BOUNDARIES = ((1018, 1019), (2042, 2043), (3066, 3067), (3446, 3447))

# ---- the case table: (extent whd, voxel size, block, azimuth, elevation) ---------------------------------------------------------------------
# voxel sizes make the box roughly cubic, so that it fills a good part of the 64x48 frame from every side
DEGENERATE = [
    ((1, 1, 1), (1, 1, 1), 1, 33.0, 20.0),
    ((2, 1, 1), (1, 2, 2), 1, 33.0, 20.0),
    ((1, 2, 1), (2, 1, 2), 1, 120.0, -25.0),
    ((1, 1, 3), (3, 3, 1), 2, 60.0, 20.0),
    ((2, 3, 1), (3, 2, 6), 1, 200.0, 35.0),
    ((3, 3, 3), (1, 1, 1), 2, 33.0, 20.0),
    ((1, 40, 30), (30, 1, 1), 4, 70.0, 15.0),
    ((37, 1, 29), (1, 30, 1), 2, 33.0, 50.0),
    ((33, 21, 1), (1, 1, 25), 4, 20.0, 20.0),
    ((2, 3, 300), (150, 100, 1), 4, 33.0, 20.0),
    ((2, 3, 300), (150, 100, 1), 1, 0.0, 0.0),          # along the long axis
]
SLABS = [
    ((1, 257, 129), (100, 1, 1), 4, 70.0, 20.0),
    ((129, 1, 257), (1, 100, 1), 3, 33.0, 55.0),
    ((257, 129, 1), (1, 1, 100), 2, 20.0, 20.0),
]
# needle: (extent, block); the long axis's voxel size is 4 / its length.  Two views each: OBLIQUE, and along the long axis - azimuth 90 for
# x, azimuth 0 for z, both at elevation 0 (the central rays are axis-parallel and run the whole length).  The orbit camera's up vector is y, so
# it has no view exactly along y: the y needles are seen from elevation 89 (the rays within the box then leave the axis by under 2 % of the
# box's width over its whole length)
_NEEDLES = [
    ((1010, 4, 4), 4), ((1011, 4, 4), 2),               # 1018 | 1019, x
    ((4, 2034, 4), 5), ((4, 2035, 4), 3),               # 2042 | 2043, y
    ((4, 3, 3059), 2), ((4, 3, 3060), 4),               # 3066 | 3067, z
    ((3440, 3, 3), 5), ((3441, 3, 3), 3),               # 3446 | 3447, x
    ((3, 3440, 3), 4), ((3, 3441, 3), 5),               # 3446 | 3447, y
    ((3, 3, 3440), 3), ((3, 3, 3441), 2),               # 3446 | 3447, z
    ((5000, 4, 4), 3),                                  # well beyond
]
ALONG = {0: (90.0, 0.0), 1: (0.0, 89.0), 2: (0.0, 0.0)}


def long_axis(whd):
    return int(np.argmax(whd))


def _needle_cases():
    out = []
    for whd, block in _NEEDLES:
        a = long_axis(whd)
        voxel = tuple(4.0 / whd[k] if k == a else 1.0 for k in range(3))
        out.append((whd, voxel, block) + OBLIQUE)
        out.append((whd, voxel, block) + ALONG[a])
    return out


NEEDLES = _needle_cases()
CASES = DEGENERATE + SLABS + NEEDLES


def case_id(case):
    whd, _, block, az, el = case
    return "%dx%dx%d-b%d-az%g-el%g" % (whd + (block, az, el))


def is_needle(case):
    return max(case[0]) >= 1000


def is_along(case):
    """the view along the long axis of a needle (or of the 2x3x300 column)"""
    return max(case[0]) >= 300 and min(case[0]) <= 4 and (case[3], case[4]) == ALONG[long_axis(case[0])]


def both_ert(case):
    """cases rendered with early ray termination on AND off (the others: on)"""
    return case in DEGENERATE or (is_needle(case) and is_along(case))


def build_scene(case):
    """The oracle scene of a case: T.random_volume(extent, seed, sparsity = 0.9) under T.APP_TF.  A volume whose gradient map is zero
    everywhere (1x1x1: under APP_TF a voxel of 255 is sampled and stays transparent) takes the no-gradient transfer function and a bright
    voxel."""
    whd, voxel, block, _, _ = case
    seed = 1000 + sum(whd) + 7 * block
    vol = T.random_volume(whd, seed, sparsity=0.9)
    # a ray takes ceil(longest axis * its length in texture space * sampling_factor) steps and needs two: at the default factor 1 all but the
    # diagonal rays of a volume of 1 .. 3 voxels take none
    sf = 8.0 if max(whd) <= 3 else 1.0
    opt = abi.VolumeOptions(sampling_factor=sf, **T.APP_TF)
    if max(whd) <= 3:
        vol.reshape(-1)[0] = 255        # (nine voxels in ten are dim: most volumes of a few voxels would have no visible one)
    if not O.gradient_map(vol, O.transfer_function_uniform(opt)).any():
        opt = abi.VolumeOptions(sampling_factor=sf, **NO_GRADIENT_TF)
        vol.reshape(-1)[0] = 255
    return T.OracleScene(vol, opt, block, voxel_size=voxel)


def case_params(scene, case, skipping_type, ert=True, uniforms=None):
    """RenderParams of a case.  uniforms None: built by the HIP library (OracleScene.params); this file passes the oracle's."""
    _, _, _, az, el = case
    view, proj = T.orbit(az, el, RADIUS, image_size=SIZE)
    ro = abi.RenderOptions(skipping_type=skipping_type, clip_distance=1.0, early_ray_termination=ert)
    return scene.params(view, proj, SIZE, ro, uniforms=uniforms)


def oracle_uniforms(scene, case):
    _, _, _, az, el = case
    view, proj = T.orbit(az, el, RADIUS, image_size=SIZE)
    return O.build_uniforms(view, proj, scene.node_transform, scene.image_transform, 1.0, SIZE, scene.extent, scene.map_extent)


# ---- premises on the table itself --------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    """the restated rule is the one in the sources"""
    csrc = T.CSRC
    core = open(os.path.join(csrc, "raymarch_core.hpp")).read()
    host = open(os.path.join(os.path.dirname(csrc), "host", "host_arith.cpp")).read()

    def const(name, text=core):
        m = re.search(r"%s\s*=\s*(\d+)" % name, text)
        assert m, name
        return int(m.group(1))

    assert const("kFullLutWord") == FULL_LUT_WORD
    assert const("kFullLdsLimit") == FULL_LDS_LIMIT
    assert const("kFullCopyRounds") == COPY_ROUNDS
    assert const(r"t\.full_table_lds_limit", host) == FULL_LDS_LIMIT
    assert "(size_t) (W + 2 + H + 2 + D + 2) * 4" in core                                 # full_lut_bytes
    assert "((uint32_t) (A.W + 2 + A.H + 2 + A.D + 2) + 3u) >> 2" in core                 # nvec: 16-byte pieces
    assert "__launch_bounds__(%d)" % WORKGROUP in core
    assert const("kLdsBase") == LDS_BASE
    assert "float    alpha[256];" in core and "uint32_t bits[2048];" in core and "float    unorm[256];" in core        # sizeof(RmLds)
    assert "kLdsBase + sizeof(RmLds) + (size_t) lut_words * 4" in core and "kLdsBase + (size_t) kFullLutWord * 4 + ((full_lut_bytes(W, H, D) + 15u) & ~(size_t) 15u)" in core
    tables = open(os.path.join(csrc, "addr_tables.hpp")).read()
    assert "nmx = (uint32_t) (W + 1) / 32 + 1" in tables and "ny = 96 + nmx, nz = (ny + nmy + 1) & ~1u, total = nz + 2 * nmz" in tables
    assert ("choices[i].kind != choices[p.ref].kind || choices[i].lds != choices[p.ref].lds || a.lut_words != frames[p.ref].lut_words"
            in open(os.path.join(csrc, "raymarch_plan.hpp")).read())                       # plan_batch: frames that disagree about the tables
    assert "kFullLutWord * 4 + full_lut_bytes(a.W, a.H, a.D)" in open(os.path.join(csrc, "raymarch.hip")).read()


def test_boundaries_have_both_sides():
    sums = {sum(c[0]) for c in NEEDLES}
    # what the boundaries ARE, from the rule: copy rounds 1, 2, 3 first have a piece at the upper value of a pair; the table kind changes at the last
    for k, (below, above) in enumerate(BOUNDARIES[:3]):
        e_lo, e_hi = (below - 2, 1, 1), (above - 2, 1, 1)
        assert copy_rounds(e_lo) == k + 1 and copy_rounds(e_hi) == k + 2, (below, above)
        assert copy_pieces(e_lo) == (k + 1) * WORKGROUP and copy_pieces(e_hi) == (k + 1) * WORKGROUP + 1
    below, above = BOUNDARIES[3]
    assert takes_per_voxel_tables((below - 2, 1, 1)) and not takes_per_voxel_tables((above - 2, 1, 1))
    assert copy_rounds((below - 2, 1, 1)) <= COPY_ROUNDS        # the unrolled rounds cover every volume that takes the per-voxel tables
    for below, above in BOUNDARIES:
        assert below in sums and above in sums, (below, above)
    assert max(sums) >= 5000 and not takes_per_voxel_tables((5000, 4, 4))
    # each axis is the long one at two boundaries or more, each boundary has both sides on one axis, and both views exist for every needle
    per_axis = {0: set(), 1: set(), 2: set()}
    for whd, _ in _NEEDLES:
        assert sorted(whd)[0] in (3, 4) and sorted(whd)[1] in (3, 4)
        for pair in BOUNDARIES:
            if sum(whd) in pair:
                per_axis[long_axis(whd)].add(pair)
    assert all(len(s) >= 2 for s in per_axis.values()), per_axis
    for whd, _ in _NEEDLES:
        views = {(c[3], c[4]) for c in NEEDLES if c[0] == whd}
        assert views == {OBLIQUE, ALONG[long_axis(whd)]}
    assert {c[2] for c in NEEDLES} == {2, 3, 4, 5} and {c[2] for c in DEGENERATE} == {1, 2, 4} and [c[2] for c in SLABS] == [4, 3, 2]
    assert any(max(c[0]) % c[2] for c in NEEDLES)        # blocks that do not divide the long axis
    assert ((3441, 3, 3), 3) in _NEEDLES and ((3, 3441, 3), 5) in _NEEDLES
    # every oracle-parity test elsewhere stays in round 0; the small cases here do too (they are about the clamps, not the copy)
    assert all(copy_rounds(c[0]) == 1 for c in DEGENERATE + SLABS)


# ---- the mixed batches of the GPU file: (name, [(extent, voxel size, block), ...], what the launcher's rule says about them) -----------------
BATCHES = [
    ("a-permuted-small", [((40, 24, 8), (1, 1.6, 5), 4), ((8, 40, 24), (5, 1, 1.6), 4)], True),
    ("a-permuted-needles-xy", [((1011, 4, 4), (0.004, 1, 1), 2), ((4, 1011, 4), (1, 0.004, 1), 2)], True),
    ("a-permuted-needles-xz", [((1011, 4, 4), (0.004, 1, 1), 2), ((4, 4, 1011), (1, 1, 0.004), 2)], False),        # z terms are 64-bit: lut_words differ
    ("b-one-and-two-copy-rounds", [((1010, 4, 4), (0.004, 1, 1), 4), ((1011, 4, 4), (0.004, 1, 1), 2)], True),
    ("b-small-different-sums", [((40, 24, 8), (1, 1.6, 5), 4), ((33, 21, 1), (1, 1, 25), 4)], True),
    ("b-needles-different-sums", [((1010, 4, 4), (0.004, 1, 1), 4), ((3440, 3, 3), (0.001, 1, 1), 5)], False),
    ("b-two-level-different-sums", [((3441, 3, 3), (0.001, 1, 1), 3), ((5000, 4, 4), (0.0008, 1, 1), 3)], False),
    ("c-needle-and-cube", [((3441, 3, 3), (0.001, 1, 1), 3), ((24, 24, 24), (1, 1, 1), 4)], False),
]


BATCH_VIEWS = ((33.0, 20.0), (200.0, -30.0))        # every volume of a batch from both


def test_batch_frames_are_not_empty():
    for whd, voxel, block in sorted({v for _, vols, _ in BATCHES for v in vols}):
        for az, el in BATCH_VIEWS:
            case = (whd, voxel, block, az, el)
            scene = build_scene(case)
            for st in SKIPS:
                ref = scene.render(case_params(scene, case, st, True, oracle_uniforms(scene, case)))
                assert float(((ref.counts[..., 0] + ref.counts[..., 1]) > 0).mean()) >= 0.10 and float(ref.color[..., 3].max()) > 0.0, (case_id(case), st)
                assert st == abi.SKIP_NONE or int(ref.counts[..., 1].sum()) > 0, (case_id(case), st)


def test_batches_cover_both_outcomes():
    for name, vols, shared in BATCHES:
        extents = [v[0] for v in vols]
        assert batch_shares_a_kernel(extents) == shared, name
        assert len(set(extents)) == len(extents), name
    by = {name: [v[0] for v in vols] for name, vols, _ in BATCHES}
    # (a) permutations of one extent, both outcomes; the shared ones stage different tables (the y and z table offsets differ)
    for name in ("a-permuted-small", "a-permuted-needles-xy", "a-permuted-needles-xz"):
        assert sorted(by[name][0]) == sorted(by[name][1])
    # (b) different W + H + D on one side of the table-kind boundary; one pair straddles a copy-round boundary inside a shared kernel
    for name in ("b-one-and-two-copy-rounds", "b-small-different-sums", "b-needles-different-sums", "b-two-level-different-sums"):
        a, b = by[name]
        assert sum(a) != sum(b) and takes_per_voxel_tables(a) == takes_per_voxel_tables(b), name
    assert [copy_rounds(e) for e in by["b-one-and-two-copy-rounds"]] == [1, 2]
    # (c) the kinds differ
    assert {lean_choice(e)[0] for e in by["c-needle-and-cube"]} == {1, 2}


def test_lut_words_is_the_builders(tmp_path):
    """lut_words() against the host-only builder itself (tests/addr_tables_driver.cpp prints build_addr_tables' offsets)"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "addr_tables_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(os.path.dirname(os.path.abspath(__file__)), "addr_tables_driver.cpp"), "-o", exe])
    for whd in sorted({v[0] for _, vols, _ in BATCHES for v in vols} | {(3, 3, 3441), (1, 1, 1)}):
        words = int(subprocess.check_output([exe] + [str(e) for e in whd], text=True).split("\n")[0].split()[2])
        assert words == lut_words(whd), whd


def test_case_ids_are_unique():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)


# ---- premises on the oracle's frames -----------------------------------------------------------------------------------------------------
_slowest = [0.0, ""]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_frames_are_not_empty(case):
    """What the GPU comparison stands on, for all four skipping types: 10 % of the pixels or more carry a sample or a probe, there are samples and
    visible pixels, with skipping there are probes (a map of one cell is never probed: a probe needs a change of cell), and along a needle the
    longest ray takes half the long axis in samples or more.  That last one is asserted on the frames without early ray termination: with it
    the rays of these views end at the first few bright voxels (399 samples at most on 3441x3x3, against 3635 without, 3470 with block skipping)."""
    t0 = time.perf_counter()
    scene = build_scene(case)
    uniforms = oracle_uniforms(scene, case)
    whd = case[0]
    me = scene.map_extent
    for st in SKIPS:
        for ert in ((True, False) if both_ert(case) else (True,)):
            ref = scene.render(case_params(scene, case, st, ert, uniforms))
            what = "%s mode %d ert %d" % (case_id(case), st, ert)
            touched = float(((ref.counts[..., 0] + ref.counts[..., 1]) > 0).mean())
            print("%s: %.0f %% of the pixels, %d samples, %d probes, %d visible, longest ray %d samples" % (
                what, 100 * touched, int(ref.counts[..., 0].sum()), int(ref.counts[..., 1].sum()), int((ref.color[..., 3] > 0).sum()),
                int(ref.counts[..., 0].max())))
            assert touched >= 0.10, what
            assert int(ref.counts[..., 0].sum()) > 0, what
            assert float(ref.color[..., 3].max()) > 0.0, what
            if st != abi.SKIP_NONE and me.width * me.height * me.depth > 1:
                assert int(ref.counts[..., 1].sum()) > 0, what
            if is_needle(case) and is_along(case) and not ert:
                assert int(ref.counts[..., 0].max()) >= max(whd) // 2, what
    dt = time.perf_counter() - t0
    if dt > _slowest[0]:
        _slowest[:] = [dt, case_id(case)]
    print("case took %.3f s on the CPU (slowest so far: %.3f s, %s)" % (dt, _slowest[0], _slowest[1]))
