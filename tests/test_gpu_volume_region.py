"""GPU: the region update of the volume (vkv_update_volume_region) against a full rebuild of the updated volume with the existing entry
points (vkv_convert_volume of the source, vkv_gradient_map, vkv_pack_volume, vkv_compute_distance_map): every byte of the volume, the
gradient, the packed image and every map in use, over volumes of odd, tiny and C3 size, block sizes, transfer-function variants, skipping
types, boxes and source types; queued updates, occupancy flips, frames, two streams, hipGraph capture, argument checks and the driver."""
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as T
from vkvolume_amd import abi, lib, volume as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vkvolume_amd", "csrc", "vkv_offscreen")
U8, I8, U16, I16 = abi.VOXEL_TYPES["uint8_t"], abi.VOXEL_TYPES["int8_t"], abi.VOXEL_TYPES["uint16_t"], abi.VOXEL_TYPES["int16_t"]
NP_TYPES = {U8: np.uint8, I8: np.int8, U16: np.uint16, I16: np.int16}
# (voxel type, big endian, normalisation range): the loader's conversions, ranges inside, around and beyond the type's
SOURCES = [(U8, False, (0.0, 255.0)), (I8, False, (-40.0, 90.0)), (U16, True, (400.0, 2538.0)), (U16, False, (0.0, 65535.0)),
           (I16, True, (-1000.0, 3000.0)), (I16, False, (-200.0, 900.0)), (U8, False, (30.0, 200.0)), (I8, True, (-128.0, 127.0))]


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def map_extent(ext, block):
    return abi.Extent3D(*[-(-n // block) for n in ext.as_tuple()])


class State:
    """Every buffer of one volume, built with the existing whole-volume entry points (the update's precondition)."""

    def __init__(self, ctx, vol, block, opts, grad_mode, packed, skip):
        self.ctx, self.block, self.opts, self.grad_mode, self.skip = ctx, block, opts, grad_mode, skip
        o = dict(opts)
        if grad_mode == "off":  # gradient_min == gradient_max: use_gradient = 0
            o["gradient_min"] = o["gradient_max"] = 0.25
        self.tf = lib.transfer_function_uniform(abi.VolumeOptions(**o))
        self.tex = torch.from_numpy(lib.transfer_function_texture(abi.VolumeOptions(**o))).cuda()
        self.vol = vol.clone()
        d, h, w = vol.shape
        self.ext = abi.Extent3D(w, h, d)
        self.mext = map_extent(self.ext, block)
        self.grad = torch.zeros_like(vol) if grad_mode != "fly" else None
        self.packed = torch.zeros(ctx.packed_volume_bytes(self.ext), dtype=torch.uint8, device="cuda") if packed else None
        me = (self.mext.depth, self.mext.height, self.mext.width)
        self.maps = [torch.zeros(me, dtype=torch.uint8, device="cuda") for _ in range(8 if skip == abi.SKIP_ANISOTROPIC_DISTANCE else 1)]
        self.swap = torch.zeros(me, dtype=torch.uint8, device="cuda")
        self.rebuild()

    def rebuild(self):
        c, s = self.ctx, st()
        if self.grad is not None:
            c.gradient_map(ptr(self.vol), ptr(self.grad), self.ext, self.tf, s)
        if self.packed is not None:
            c.pack_volume(ptr(self.vol), ptr(self.grad), self.ext, ptr(self.packed), s)
        c.compute_distance_map(ptr(self.vol), ptr(self.grad), ptr(self.tex), self.tf, self.ext, [ptr(m) for m in self.maps], ptr(self.swap),
                               self.mext, self.skip, s)

    def args(self, src, source, box):
        vt, big, (lo, hi) = source
        return [ptr(src), vt, big, lo, hi, box, ptr(self.vol), ptr(self.grad), ptr(self.packed), self.ext, ptr(self.tex), self.tf,
                [ptr(m) for m in self.maps], ptr(self.swap), self.mext, self.skip]

    def update(self, src, source, box, stream=None):
        self.ctx.update_volume_region(*self.args(src, source, box), stream=st() if stream is None else stream)

    def buffers(self):
        out = [("volume", self.vol), ("gradient", self.grad), ("packed", self.packed)]
        return out + [("map%d" % i, m) for i, m in enumerate(self.maps)]

    def snapshot(self):
        return [(n, None if t is None else t.clone()) for n, t in self.buffers()]


def make_source(rng, source, box, empty_share=0.0):
    """Raw elements of the source's type for the box (x fastest), as a device tensor; values around the normalisation range."""
    vt, _, (lo, hi) = source
    info = np.iinfo(NP_TYPES[vt])
    span = hi - lo
    vals = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(box.depth, box.height, box.width))
    if empty_share > 0:
        vals[rng.random(vals.shape) < empty_share] = lo
    raw = np.clip(np.rint(vals), info.min, info.max).astype(NP_TYPES[vt])
    if rng.random() < 0.3:  # some raw bit patterns outright (byte-swapped values, extremes)
        raw = rng.integers(info.min, info.max, size=raw.shape, endpoint=True).astype(NP_TYPES[vt])
    if raw.dtype == np.uint16:
        raw = raw.view(np.int16)
    return torch.from_numpy(np.ascontiguousarray(raw)).cuda()


def expected_volume(ctx, vol, src, source, box):
    """The updated volume: the source converted by vkv_convert_volume, placed into the box."""
    vt, big, (lo, hi) = source
    n = box.width * box.height * box.depth
    conv = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.convert_volume(ptr(src), vt, big, lo, hi, n, ptr(conv), st())
    out = vol.clone()
    out[box.z0:box.z0 + box.depth, box.y0:box.y0 + box.height, box.x0:box.x0 + box.width] = conv.view(box.depth, box.height, box.width)
    return out


def mismatches(state, exp_vol):
    """Names of the buffers of `state` that differ from a full rebuild of exp_vol (compared on the device)."""
    ref = State(state.ctx, exp_vol, state.block, state.opts, state.grad_mode, state.packed is not None, state.skip)
    bad = []
    for (name, got), (_, want) in zip(state.buffers(), ref.buffers()):
        if got is not None and not torch.equal(got, want):
            bad.append("%s (%d bytes)" % (name, int((got != want).sum().item())))
    return bad


def boxes(ext, rng, n_random=4):
    """A single voxel inside and at the 8 corners, a full x row, a z slab, a box flush with the far faces, the whole volume, random boxes."""
    w, h, d = ext.as_tuple()
    out = [abi.Box(w // 2, h // 2, d // 2, 1, 1, 1)]
    for cx, cy, cz in itertools.product((0, w - 1), (0, h - 1), (0, d - 1)):
        out.append(abi.Box(cx, cy, cz, 1, 1, 1))
    out.append(abi.Box(0, h // 3, d // 2, w, 1, 1))
    z0 = d // 3
    out.append(abi.Box(0, 0, z0, w, h, min(d - z0, 5)))
    x0, y0, z0 = w // 2, h // 3, d // 4
    out.append(abi.Box(x0, y0, z0, w - x0, h - y0, d - z0))
    out.append(abi.Box(0, 0, 0, w, h, d))
    for _ in range(n_random):
        size = [int(rng.integers(1, max(2, n // 2) + 1)) for n in (w, h, d)]
        org = [int(rng.integers(0, n - s + 1)) for n, s in zip((w, h, d), size)]
        out.append(abi.Box(*org, *size))
    return out


def start_volume(ctx, shape_whd, seed):
    w, h, d = shape_whd
    vol = torch.empty((d, h, w), dtype=torch.uint8, device="cuda")
    if w >= 16 and h >= 16 and d >= 16:
        ctx.synth_volume(ptr(vol), abi.Extent3D(w, h, d), 1, seed, st())
    else:
        vol.copy_(torch.from_numpy(T.random_volume(shape_whd, seed, sparsity=0.5)))
    return vol


# ---- 1. the matrix -----------------------------------------------------------------------------------------------------------------
# (shape, block sizes): not divisible by the block, 4 and 3 voxels wide, the synthetic shell scene
VOLUMES = [((37, 29, 23), (3, 2, 4, 6)), ((4, 21, 19), (2, 3, 6)), ((3, 17, 13), (2, 3)), ((256, 192, 160), (4, 6, 3))]
VARIANTS = [("precomputed", True), ("precomputed", False), ("fly", True), ("off", True)]  # gradient mode, packed image
SKIPS = [abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE]


@pytest.mark.parametrize("shape,blocks", VOLUMES, ids=["%dx%dx%d" % s for s, _ in VOLUMES])
def test_region_update_equals_full_rebuild(ctx, shape, blocks):
    rng = np.random.default_rng(sum(shape))
    base = start_volume(ctx, shape, 0xB0C5 + shape[0])
    bad, k = [], 0
    for block, (grad_mode, packed), skip in itertools.product(blocks, VARIANTS, SKIPS):
        s = State(ctx, base, block, T.APP_TF, grad_mode, packed, skip)
        exp = s.vol.clone()
        for j, box in enumerate(boxes(s.ext, rng, n_random=8)):
            source = SOURCES[(k + j) % len(SOURCES)]
            src = make_source(rng, source, box, empty_share=0.5 if j % 3 == 0 else 0.0)
            exp = expected_volume(ctx, exp, src, source, box)
            s.update(src, source, box)
            m = mismatches(s, exp)
            if m:
                bad.append("block %d %s packed=%s skip %d box %s source %s: %s" % (
                    block, grad_mode, packed, skip, (box.x0, box.y0, box.z0, box.width, box.height, box.depth), source, ", ".join(m)))
                s = State(ctx, exp, block, T.APP_TF, grad_mode, packed, skip)  # go on from a valid state
        k += 1
    torch.cuda.synchronize()
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("skip", [abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_region_update_equals_full_rebuild_c3_size(ctx, skip):
    rng = np.random.default_rng(skip)
    base = start_volume(ctx, (1024, 1024, 795), 0xC0FFEE03)
    s = State(ctx, base, 4, T.APP_TF, "precomputed", True, skip)
    del base
    exp = s.vol.clone()
    w, h, d = s.ext.as_tuple()
    cases = [abi.Box(500, 600, 400, 1, 1, 1), abi.Box(300, 200, 100, 128, 128, 128), abi.Box(0, 0, 700, w, h, 64),
             abi.Box(w - 77, h - 55, d - 33, 77, 55, 33)]
    bad = []
    for j, box in enumerate(cases):
        source = SOURCES[(j + skip) % len(SOURCES)]
        src = make_source(rng, source, box, empty_share=0.5)
        exp = expected_volume(ctx, exp, src, source, box)
        s.update(src, source, box)
        m = mismatches(s, exp)
        torch.cuda.empty_cache()
        if m:
            bad.append("box %d: %s" % (j, ", ".join(m)))
    assert not bad, "\n".join(bad)


# ---- 2. queued updates -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", SKIPS)
def test_25_queued_updates_compared_once(ctx, skip):
    rng = np.random.default_rng(25 + skip)
    s = State(ctx, start_volume(ctx, (61, 47, 39), 0x25), 3, T.APP_TF, "precomputed", True, skip)
    exp = s.vol.clone()
    torch.cuda.synchronize()
    for j in range(25):  # no synchronisation in between
        size = [int(rng.integers(1, 20)) for _ in range(3)]
        org = [int(rng.integers(0, n - z + 1)) for n, z in zip(s.ext.as_tuple(), size)]
        box = abi.Box(*org, *size)
        source = SOURCES[j % len(SOURCES)]
        src = make_source(rng, source, box, empty_share=0.6 if j % 2 else 0.0)
        exp = expected_volume(ctx, exp, src, source, box)
        s.update(src, source, box)
    m = mismatches(s, exp)
    assert not m, m


# ---- 3. occupancy flips both ways ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", SKIPS)
def test_occupancy_flips_both_ways(ctx, skip):
    vol = torch.zeros((40, 48, 64), dtype=torch.uint8, device="cuda")
    vol[8:16, 10:20, 20:30] = 200  # the only occupied region
    s = State(ctx, vol, 4, T.APP_TF, "precomputed", True, skip)
    occ = s.maps[-1] if skip == abi.SKIP_ANISOTROPIC_DISTANCE else s.maps[0]
    assert int((occ == 0).sum()) > 0
    clear = abi.Box(19, 9, 7, 12, 12, 10)
    src = torch.zeros((clear.depth, clear.height, clear.width), dtype=torch.uint8, device="cuda")
    s.update(src, SOURCES[0], clear)
    exp = expected_volume(ctx, s.vol, src, SOURCES[0], clear)
    assert not mismatches(s, exp)
    assert all(int((m == 0).sum()) == 0 for m in s.maps), "a cell is still occupied"
    if skip >= abi.SKIP_DISTANCE:
        assert all(int(m.min()) > 1 for m in s.maps)
    fill = abi.Box(40, 30, 25, 9, 7, 6)
    src = torch.full((fill.depth, fill.height, fill.width), 230, dtype=torch.uint8, device="cuda")
    exp = expected_volume(ctx, exp, src, SOURCES[0], fill)
    s.update(src, SOURCES[0], fill)
    assert not mismatches(s, exp)
    assert int((occ == 0).sum()) > 0


# ---- 4. frames -------------------------------------------------------------------------------------------------------------------
def full_volume(ctx, vol_np, skip):
    v = V.Volume(ctx)
    v.options = abi.VolumeOptions(**T.APP_TF)
    v.load_from_array(vol_np, 4)
    V.default_scene(v)
    tf = v.get_transfer_function_uniform()
    V.ComputeGradientMap(ctx).compute(v, tf)
    v.update_transfer_function_texture()
    V.ComputeDistanceMap(ctx).compute(v, tf, skip)
    return v


def render_batch(ctx, v, skip, size=(160, 96)):
    sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=skip, clip_distance=1.0), size)
    rgba8 = torch.zeros((size[1], size[0], 4), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((size[1], size[0], 3), dtype=torch.int32, device="cuda")
    ps = []
    for az in (30.0, 130.0):
        view, proj = T.orbit(az, image_size=size)
        p = sp.make_params(view, proj)
        ps.append(p)
    outs = [(rgba8.clone(), counts.clone()) for _ in ps]
    for p, (c, n) in zip(ps, outs):
        p.d_out_rgba8, p.d_out_counts = c.data_ptr(), n.data_ptr()
    ctx.render_batch(ps, st())
    torch.cuda.synchronize()
    return [(c.cpu().numpy(), n.cpu().numpy()) for c, n in outs]


@pytest.mark.parametrize("skip", [abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_frames_after_updates_equal_frames_of_the_rebuilt_volume(ctx, skip):
    rng = np.random.default_rng(40 + skip)
    vol = T.random_volume((96, 80, 72), 7, sparsity=0.9)
    v = full_volume(ctx, vol, skip)
    render_batch(ctx, v, skip)  # packs the volume
    for j in range(4):
        size = [int(rng.integers(4, 40)) for _ in range(3)]
        org = [int(rng.integers(0, n - z + 1)) for n, z in zip((96, 80, 72), size)]
        new = rng.integers(0, 256, size=size[::-1], dtype=np.uint8)
        if j % 2:
            new[:] = 0
            v.update_region(org, new, skip)
        else:
            v.update_region(org, torch.from_numpy(new).cuda(), skip)  # a device tensor
        vol[org[2]:org[2] + size[2], org[1]:org[1] + size[1], org[0]:org[0] + size[0]] = new
    got = render_batch(ctx, v, skip)
    ref_v = full_volume(ctx, vol, skip)
    want = render_batch(ctx, ref_v, skip)
    assert np.array_equal(v.volume.cpu().numpy(), vol)
    assert want[0][1][..., 0].sum() > 0
    for (gc, gn), (wc, wn) in zip(got, want):
        assert np.array_equal(gc, wc) and np.array_equal(gn, wn)


# ---- 5. streams and graphs ---------------------------------------------------------------------------------------------------------
def test_two_volumes_updated_on_two_streams(ctx):
    rng = np.random.default_rng(2)
    states = [State(ctx, start_volume(ctx, (80, 64, 48), 0x51 + i), 4, T.APP_TF, "precomputed", True, abi.SKIP_ANISOTROPIC_DISTANCE)
              for i in range(2)]
    plans = []
    for s in states:
        exp, steps = s.vol.clone(), []
        for j in range(6):
            size = [int(rng.integers(1, 30)) for _ in range(3)]
            org = [int(rng.integers(0, n - z + 1)) for n, z in zip(s.ext.as_tuple(), size)]
            box, source = abi.Box(*org, *size), SOURCES[j]
            src = make_source(rng, source, box, empty_share=0.5)
            exp = expected_volume(ctx, exp, src, source, box)
            steps.append((src, source, box))
        plans.append((exp, steps))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for j in range(6):
        for s, (_, steps), stream in zip(states, plans, streams):
            s.update(*steps[j], stream=stream.cuda_stream)
    torch.cuda.synchronize()
    for s, (exp, _) in zip(states, plans):
        assert not mismatches(s, exp)
    for stream in streams:
        ctx.release_stream(stream.cuda_stream)


def test_update_captured_into_a_graph(ctx):
    rng = np.random.default_rng(3)
    s = State(ctx, start_volume(ctx, (72, 56, 40), 0x6A), 3, T.APP_TF, "precomputed", True, abi.SKIP_DISTANCE)
    first, second = abi.Box(5, 6, 7, 20, 10, 8), abi.Box(40, 30, 20, 25, 20, 15)
    src1 = make_source(rng, SOURCES[2], first, 0.5)
    src2 = make_source(rng, SOURCES[4], second, 0.5)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):  # one direct call: the stream's scratch block exists
        s.update(src1, SOURCES[2], first)
    torch.cuda.synchronize()
    exp = expected_volume(ctx, s.vol, src2, SOURCES[4], second)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        s.update(src2, SOURCES[4], second)
    torch.cuda.synchronize()
    assert not torch.equal(s.vol, exp)  # the capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert not mismatches(s, exp)
    del g
    ctx.release_stream(stream.cuda_stream)


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(ctx):
    E = abi.VKV_E_INVALID_ARGUMENT
    s = State(ctx, start_volume(ctx, (24, 20, 16), 0x77), 4, T.APP_TF, "precomputed", True, abi.SKIP_ANISOTROPIC_DISTANCE)
    box = abi.Box(2, 3, 4, 5, 6, 7)
    src16 = torch.full((box.width * box.height * box.depth + 1,), 1234, dtype=torch.int16, device="cuda")
    good = s.args(src16, SOURCES[2], box)
    mp = good[12]
    # State.args: 0 source, 1 type, 5 box, 6 volume, 8 packed, 9 extent, 10 texture, 11 tf, 12 maps, 13 swap, 14 map extent, 15 skipping type
    cases = {"null source": {0: None}, "misaligned 16-bit source": {0: good[0] + 1}, "unknown type": {1: 4}, "negative type": {1: -1},
             "null box": {5: None}, "empty box": {5: abi.Box(2, 3, 4, 0, 6, 7)}, "box past the width": {5: abi.Box(20, 3, 4, 5, 6, 7)},
             "box past the depth": {5: abi.Box(0, 0, 10, 1, 1, 7)}, "box wraps in 32 bits": {5: abi.Box(0xFFFFFFF0, 0, 0, 0x20, 1, 1)},
             "null volume": {6: None}, "misaligned packed image": {8: good[8] + 16}, "zero extent": {9: abi.Extent3D(24, 0, 16)},
             "null texture": {10: None}, "null tf": {11: None}, "null map": {12: mp[:7] + [None]}, "null swap": {13: None},
             "swap aliases a map": {13: mp[2]}, "map extent above the volume": {14: abi.Extent3D(25, 5, 4)},
             "zero map extent": {14: abi.Extent3D(6, 0, 4)}, "bad skipping type": {15: 4}, "negative skipping type": {15: -1},
             "distance without swap": {12: [mp[0]], 13: None, 15: abi.SKIP_DISTANCE},
             "distance swap aliases map 0": {12: [mp[0]], 13: mp[0], 15: abi.SKIP_DISTANCE}}
    before = s.snapshot()
    for label, change in cases.items():
        a = list(good)
        for i, val in change.items():
            a[i] = val
        rc = ctx.update_volume_region_rc(*a, stream=st())
        assert rc == E, "%s: rc %d" % (label, rc)
    # map rows too long for the distance transform (VKV_E_UNSUPPORTED), refused before anything is enqueued
    e = abi.Extent3D(2049, 1, 1)
    wide = [torch.full((1, 1, 2049), 7, dtype=torch.uint8, device="cuda") for _ in range(4)]  # volume, gradient, map, swap
    src8 = torch.full((1,), 200, dtype=torch.uint8, device="cuda")
    rc = ctx.update_volume_region_rc(ptr(src8), U8, False, 0.0, 255.0, abi.Box(0, 0, 0, 1, 1, 1), ptr(wide[0]), ptr(wide[1]), None, e,
                                     good[10], good[11], [ptr(wide[2])], ptr(wide[3]), e, abi.SKIP_DISTANCE, stream=st())
    assert rc == abi.VKV_E_UNSUPPORTED and ctx.last_error().startswith("update_volume_region:"), rc
    torch.cuda.synchronize()
    for (name, b), (_, a) in zip(before, s.snapshot()):
        assert b is None or torch.equal(a, b), "%s changed by a rejected call" % name
    assert all((t == 7).all() for t in wide)
    assert ctx.update_volume_region_rc(*good, stream=st()) == abi.VKV_OK  # the unchanged arguments are accepted
    torch.cuda.synchronize()


# ---- 7. the driver ---------------------------------------------------------------------------------------------------------------
def offscreen(args, out):
    r = subprocess.run([EXE, "--width=160", "--height=112", "--dump-rgba8=%s" % out] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, out.read_bytes()


@pytest.mark.parametrize("skipmode", [2, 3])
def test_offscreen_stream_slabs_equal_one_shot_load(tmp_path, skipmode):
    assert os.path.exists(EXE), "vkv_offscreen not built (run __graft_entry__.build())"
    w, h, d = 48, 40, 35
    raw = np.random.default_rng(9).integers(0, 3000, size=(d, h, w)).astype(">u2")
    raw[:, :, : w // 3] = 100  # an empty third
    (tmp_path / "scan.raw").write_bytes(raw.tobytes())
    (tmp_path / "scan.raw.header").write_text("%d %d %d # extents\n0.001 0.001 0.002 # voxel size\n400.0 2538.0 # normalisation range\n"
                                              "uint16_t big # type\n1 0 0 90 # rotation\n" % (w, h, d))
    for source in ([str(tmp_path / "scan.raw")], ["--synthetic=72x64x56:1:7"]):
        one, f1 = offscreen(source + ["--skipmode=%d" % skipmode], tmp_path / "one.rgba")
        out, f4 = offscreen(source + ["--skipmode=%d" % skipmode, "--stream-slabs=4"], tmp_path / "slabs.rgba")
        assert "stream-slabs: 4 slabs" in out, out
        assert len(f1) == 160 * 112 * 4 and f1 == f4 and any(f1)
