"""Shared scene construction for the parity tests: the same call order as the reference's
VolumeRender::prepare (src/volume_render.cpp:186-238): load -> gradient -> TF texture -> occupancy/distance -> render."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import vkv_oracle as O
from vkvolume_amd import abi, camera, lib

APP_TF = dict(intensity_min=0.1, intensity_max=1.0, gradient_min=0.0, gradient_max=0.2)  # src/volume_render.cpp:67-70


def random_volume(shape_whd, seed, sparsity=0.0):
    """Random bytes with some smooth structure; `sparsity` = fraction of voxels forced below the app TF threshold."""
    w, h, d = shape_whd
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, size=(d, h, w), dtype=np.uint8)
    if sparsity > 0:
        mask = rng.random((d, h, w)) < sparsity
        v[mask] = rng.integers(0, 20, size=int(mask.sum()), dtype=np.uint8)
    return v


class OracleScene:
    """CPU-side scene evaluated with the oracle (the expected values of every parity test)."""

    def __init__(self, vol_dhw, options, block=4, voxel_size=(1, 1, 1), axis_angle=(1, 0, 0, 0)):
        self.vol = np.ascontiguousarray(vol_dhw, np.uint8)
        d, h, w = self.vol.shape
        self.extent = abi.Extent3D(w, h, d)
        self.block = block
        self.map_extent = O.map_extent(self.extent, block)
        self.options = options
        self.tf = O.transfer_function_uniform(options)
        self.tex = O.transfer_function_texture(options)
        self.grad = O.gradient_map(self.vol, self.tf) if options.use_precomputed_gradient else None
        self.image_transform = camera.image_transform(voxel_size, (w, h, d), axis_angle)
        self.node_transform = camera.benchmark_node_transform(self.image_transform)
        self._maps = {}

    def maps(self, skipping_type):
        if skipping_type not in self._maps:
            self._maps[skipping_type] = O.compute_distance_map(self.vol, self.grad, self.tex, self.tf, self.block, skipping_type)
        return self._maps[skipping_type]

    def params(self, view, proj, image_size, render_options, tiles=None, uniforms=None):
        w, h = image_size
        if uniforms is None:
            uniforms = lib.build_uniforms(view, proj, self.node_transform, self.image_transform, render_options.clip_distance,
                                          (w, h), self.extent, self.map_extent)
        p = abi.RenderParams()
        p.camera, p.ray_cast, p.ray_gen = uniforms
        p.transfer_function = self.tf
        p.options = render_options
        p.use_precomputed_gradient = self.options.use_precomputed_gradient
        p.image_width, p.image_height = w, h
        p.tiles = tiles if tiles is not None else abi.full_frame_tiles(w, h)
        p.volume_extent, p.map_extent = self.extent, self.map_extent
        return p

    def render(self, params, **kw):
        st = params.options.skipping_type
        maps = None if st == abi.SKIP_NONE else self.maps(st)
        return O.render(params, self.vol, self.grad, self.tex, maps, **kw)


def orbit(azimuth, elevation=20.0, radius=150.0, fov=60.0, image_size=(256, 256)):
    view = camera.orbit_camera(azimuth, elevation, radius)
    proj = camera.perspective_vulkan(fov, image_size[0] / image_size[1])
    return view, proj


def brute_force_chebyshev(occ):
    """min(255, Chebyshev distance to the nearest occupied (== 0) cell); SURVEY.md §4 KAT 1."""
    occ = np.asarray(occ)
    pts = np.argwhere(occ == 0)
    out = np.full(occ.shape, 255, np.int64)
    if len(pts) == 0:
        return out.astype(np.uint8)
    zz, yy, xx = np.indices(occ.shape)
    for (z, y, x) in pts:
        d = np.maximum(np.maximum(np.abs(zz - z), np.abs(yy - y)), np.abs(xx - x))
        out = np.minimum(out, d)
    return np.minimum(out, 255).astype(np.uint8)


def brute_force_chebyshev_octant(occ, k):
    """One-sided KAT: nearest occupied cell o with s*(o - c) >= 0 per axis, s = octant signs of map index k
    (k = (dz<0) + 2(dy<0) + 4(dx<0)); SURVEY.md §4 KAT 1."""
    sz = -1 if (k & 1) else 1
    sy = -1 if (k & 2) else 1
    sx = -1 if (k & 4) else 1
    occ = np.asarray(occ)
    pts = np.argwhere(occ == 0)
    out = np.full(occ.shape, 255, np.int64)
    zz, yy, xx = np.indices(occ.shape)
    for (z, y, x) in pts:
        dz, dy, dx = sz * (z - zz), sy * (y - yy), sx * (x - xx)
        ok = (dz >= 0) & (dy >= 0) & (dx >= 0)
        d = np.maximum(np.maximum(dz, dy), dx)
        out = np.where(ok, np.minimum(out, d), out)
    return np.minimum(out, 255).astype(np.uint8)


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vkvolume_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def kernel_listing(source, out):
    """Compiles vkvolume_amd/csrc/<source> (a file of the Makefile's SRCS) for gfx950 with the Makefile's FLAGS into the listing `out`
    (hipcc cross-compiles without a GPU; skips the test without hipcc); {kernel: {"NumVgprs": n, "ScratchSize": n}}."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^(SRCS|RMINST)\s*:=.*\b%s\b" % re.escape(source), text, flags=re.M), source
    flags = [f.replace("$(ARCH)", "gfx950") for f in re.search(r"^FLAGS\s*:=\s*(.*)$", text, flags=re.M).group(1).split() if not f.startswith("$(")]
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + flags + ["--offload-arch=gfx950", "-S", "--cuda-device-only", os.path.join(CSRC, source), "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    kernels, name = {}, None
    for line in open(out):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        m = re.match(r";\s*(NumVgprs|ScratchSize):\s*(\d+)", line)
        if m and name:
            kernels.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return kernels


def compact_pixels(size, tiles):
    """(index into the launch's compact tile buffers, index into the image) of every pixel of the image that the schedule `tiles` (an
    abi.TileSchedule with compact = 1) renders: entry k is tile tile_first + k * tile_stride of the rectangle (row-major; all zero: the whole
    image), whose pixel (lx, ly) lies at (k * tile_height + ly) * tile_width + lx"""
    w, h = size
    tw, th, r = tiles.tile_width, tiles.tile_height, tiles.rect
    x0, y0, cols = (r.x0, r.y0, r.w) if r.w and r.h else (0, 0, (w + tw - 1) // tw)
    k, ly, lx = np.meshgrid(np.arange(tiles.tile_count), np.arange(th), np.arange(tw), indexing="ij")
    t = tiles.tile_first + k * tiles.tile_stride
    px, py = (x0 + t % cols) * tw + lx, (y0 + t // cols) * th + ly
    ok = (px < w) & (py < h)
    return ((k * th + ly) * tw + lx)[ok], (py * w + px)[ok]


def stretched_orbit(azimuth, elevation, radius, image_size, stretch, fov=60.0):
    """orbit() with a projection whose aspect is `stretch` times the image's: a pixel step in x covers `stretch` times the angle of one in y"""
    return camera.orbit_camera(azimuth, elevation, radius), camera.perspective_vulkan(fov, stretch * image_size[0] / image_size[1])


def wave_patch_log2(p):
    """log2 of the width of a wave's 64-pixel patch for the view of RenderParams p (2, 3, 4: 4x16, 8x8, 16x4 pixels): the voxels a pixel step
    in x covers against one in y, in double precision, with the thresholds 1.6 and 1 / 1.6.  A test that asserts it checks its own premise
    (the view asks for that shape), not the kernel: every patch shape gives the same frame."""
    dim = np.array([p.volume_extent.width, p.volume_extent.height, p.volume_extent.depth], np.float64)
    vx, vy = (float(np.sum((np.array(list(d)[:3], np.float64) * dim) ** 2)) for d in (p.ray_gen.ddx, p.ray_gen.ddy))
    q = np.sqrt(vx / vy) if vx > 0.0 and vy > 0.0 else 1.0
    return 2 if q >= 1.6 else (4 if q <= 1.0 / 1.6 else 3)


GUARD_BYTES = 256


class Guarded:
    """Handle of a guarded() buffer: `buf` is the whole allocation (uint8), bytes [start, stop) of it are the payload, every other byte
    is a guard that was filled with `fill`."""

    def __init__(self, buf, start, stop, fill):
        self.buf, self.start, self.stop, self.fill = buf, start, stop, fill

    def check(self):
        """Indices (into the allocation) of the guard bytes that no longer hold the fill; empty when nothing strayed."""
        whole = self.buf.cpu().numpy()
        bad = np.flatnonzero(whole != self.fill)
        return [int(i) for i in bad if not self.start <= i < self.stop]


def guarded(array_or_shape, offset=0, fill=0, device="cpu", dtype=np.uint8):
    """A buffer inside ONE allocation laid out as [256 guard bytes + offset | payload | 256 guard bytes], the payload starting `offset` bytes
    past a 256-byte boundary; the whole allocation, payload included, is pre-filled with the byte `fill`.  `array_or_shape`: a numpy array or
    torch tensor (copied into the payload) or a shape of `dtype` elements (the payload keeps the fill: an output that every byte of which
    must be written).  Returns (payload view, Guarded handle).  A kernel that strays by a few bytes lands in memory the test owns and
    shows in handle.check(); nothing relies on a fault."""
    import torch
    src = None
    if isinstance(array_or_shape, torch.Tensor):
        src = array_or_shape.contiguous()
        shape, tdtype = tuple(src.shape), src.dtype
    elif isinstance(array_or_shape, np.ndarray):
        src = torch.from_numpy(np.ascontiguousarray(array_or_shape))
        shape, tdtype = tuple(src.shape), src.dtype
    else:
        shape = (array_or_shape,) if isinstance(array_or_shape, int) else tuple(array_or_shape)
        tdtype = torch.from_numpy(np.zeros(1, dtype)).dtype
    item = torch.empty(0, dtype=tdtype).element_size()
    nbytes = item * int(np.prod(shape, dtype=np.int64))
    assert 0 <= offset and offset % item == 0, "offset %d is no multiple of the element size %d" % (offset, item)
    # 255 spare bytes: the allocator promises less than 256-byte alignment on some devices (the CPU: 64)
    buf = torch.full((255 + GUARD_BYTES + offset + nbytes + GUARD_BYTES,), fill, dtype=torch.uint8, device=device)
    start = (-buf.data_ptr()) % 256 + GUARD_BYTES + offset
    view = buf[start:start + nbytes].view(tdtype).view(shape)
    if src is not None:
        view.copy_(src)
    assert view.data_ptr() % 256 == offset % 256 and view.data_ptr() == buf.data_ptr() + start
    assert start >= GUARD_BYTES and buf.numel() - (start + nbytes) >= GUARD_BYTES
    return view, Guarded(buf, start, start + nbytes, fill)
