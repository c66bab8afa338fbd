"""Host-side mirror of the reference's operator interface for the hot path, on torch device tensors.

Same names, argument meaning and call order as the reference (LDeakin/VkVolume):

* ``Volume``                — src/volume_component.h:31-93 (resource owner + ``Options`` + TF texture)
* ``ComputeGradientMap``    — src/compute_gradient_map.h:38
* ``ComputeDistanceMap``    — src/compute_distance_map.h:38
* ``VolumeRenderSubpass``   — src/volume_render_subpass.h:58-88 (``Options``, ``draw``)

torch is plumbing only (device memory + the current HIP stream); every computation goes through the C ABI.
"""
import ctypes as C

import numpy as np
import torch

from . import abi, camera, geodesic, lib
from . import labels as label_tables


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as_box(box):
    """an abi.Box from an abi.Box or ((x0, y0, z0), (width, height, depth)); None stays None"""
    if box is None or isinstance(box, abi.Box):
        return box
    (x0, y0, z0), (w, h, d) = box
    return abi.Box(x0, y0, z0, w, h, d)


class ComponentStats:
    """The records of vkv_component_stats on the device: ``raw`` is the uint8 tensor [K, 80] the call wrote (record k - 1: label k); every
    view below is computed from it by torch on the device, without a host wait.  A label that no voxel carries has voxels 0, bbox_min
    0xffffffff, bbox_max 0 and NaN centroid, mean and variance."""

    def __init__(self, raw):
        self.raw = raw
        self._u64 = raw.view(torch.int64)  # [K, 10]; 4 .. 9 are the record's uint64 fields (every sum of a real volume is below 2^63)

    def _u32(self, first, last):
        """the record's uint32 fields first .. last - 1 (of eight) as int64 [K, last - first]"""
        return self.raw.view(torch.int32)[:, first:last].to(torch.int64) & 0xffffffff

    def __len__(self):
        return self.raw.shape[0]

    @property
    def bbox_min(self):
        """int64 [K, 3]: (min_x, min_y, min_z), volume coordinates, inclusive"""
        return self._u32(0, 3)

    @property
    def bbox_max(self):
        """int64 [K, 3]: (max_x, max_y, max_z), volume coordinates, inclusive"""
        return self._u32(3, 6)

    @property
    def min_value(self):
        return self._u32(6, 7)[:, 0]

    @property
    def max_value(self):
        return self._u32(7, 8)[:, 0]

    @property
    def voxels(self):
        """int64 [K]"""
        return self._u64[:, 4]

    @property
    def centroid(self):
        """float64 [K, 3]: (sum_x, sum_y, sum_z) / voxels, volume coordinates"""
        return self._u64[:, 5:8].to(torch.float64) / self.voxels.to(torch.float64)[:, None]

    @property
    def mean(self):
        """float64 [K]: sum_value / voxels, in bytes"""
        return self._u64[:, 8].to(torch.float64) / self.voxels.to(torch.float64)

    @property
    def variance(self):
        """float64 [K]: sum_value2 / voxels - mean^2"""
        m = self.mean
        return self._u64[:, 9].to(torch.float64) / self.voxels.to(torch.float64) - m * m

    def numpy(self):
        """the records as a numpy structured array of abi.component_stats_dtype() (a copy to the host: it waits for the stream)"""
        return self.raw.cpu().numpy().view(abi.component_stats_dtype()).reshape(-1)


class Volume:
    """Owns the volume / gradient / transfer-function / distance-map device buffers
    (Volume::Image members, src/volume_component.h:87-90)."""

    def __init__(self, ctx, name="volume", device=None):
        self.ctx = ctx
        self.name = name
        self.device = torch.device("cuda", ctx.device) if device is None else device
        self.options = abi.VolumeOptions()  # Volume::Options defaults
        self.image_transform = np.eye(4, dtype=np.float32)
        self.node_transform = np.eye(4, dtype=np.float32)
        self.volume = self.gradient = self.transfer_function = None
        self.packed = self.transfer_function_bits = None  # device-internal accelerators (vkv_pack_volume, vkv_transfer_function_bits)
        self.use_packed = True
        self.distance_maps = []
        self.distance_map_swap = None
        self.extent = self.map_extent = None
        self.cell_summary = None  # vkv_cell_summary of the current volume (build_cell_summary), kept current by update_region
        self.max_map = None  # vkv_max_map of the current volume (build_max_map), kept current by update_region
        self.label_visibility_map = None  # vkv_label_visibility_map of the labels and table last given to build_label_visibility_map

    # -- load_from_file's device half (src/volume_component.cpp:55-153): take voxels, allocate images --
    def load_from_array(self, voxels_dhw, distance_map_block_size=4, image_transform=None):
        v = torch.as_tensor(np.ascontiguousarray(voxels_dhw, np.uint8)) if not torch.is_tensor(voxels_dhw) else voxels_dhw
        self.volume = v.to(self.device).contiguous()
        return self._allocate(distance_map_block_size, image_transform)

    def load_synthetic(self, extent_whd, kind, seed, distance_map_block_size=4, image_transform=None):
        w, h, d = extent_whd
        self.volume = torch.empty((d, h, w), dtype=torch.uint8, device=self.device)
        self.ctx.synth_volume(_ptr(self.volume), abi.Extent3D(w, h, d), kind, seed, _stream())
        return self._allocate(distance_map_block_size, image_transform)

    def _allocate(self, block, image_transform):
        d, h, w = self.volume.shape
        self.extent = abi.Extent3D(w, h, d)
        rnd = lambda x: (x + block - 1) // block  # noqa: E731  (volume_component.cpp:91-92)
        self.map_extent = abi.Extent3D(rnd(w), rnd(h), rnd(d))
        if self.options.use_precomputed_gradient:
            self.gradient = torch.zeros_like(self.volume)
        self.gradient_valid = False  # set by ComputeGradientMap.compute; the packed image must not be built from an empty map
        self.transfer_function = torch.zeros((256, 256, 4), dtype=torch.uint8, device=self.device)
        self.transfer_function_bits = torch.zeros(abi.TF_BITS_WORDS, dtype=torch.int32, device=self.device)
        self.packed = self.cell_summary = self.max_map = self.label_visibility_map = None
        self.distance_map_swap = torch.empty((self.map_extent.depth, self.map_extent.height, self.map_extent.width),
                                             dtype=torch.uint8, device=self.device)
        self.distance_maps = []
        if image_transform is not None:
            self.set_image_transform(image_transform)
        return True

    def set_image_transform(self, mat):
        self.image_transform = np.ascontiguousarray(mat, np.float32).reshape(4, 4)

    def set_number_of_distance_maps(self, n):
        """grow-only, re-creates all maps when growing (src/volume_component.cpp:155-184)"""
        if n <= len(self.distance_maps):
            return
        self.distance_maps = [torch.empty_like(self.distance_map_swap) for _ in range(n)]

    def get_transfer_function_uniform(self):
        return lib.transfer_function_uniform(self.options)

    def update_transfer_function_texture(self):
        tex = lib.transfer_function_texture(self.options)  # CPU builds the LUT (volume_component.cpp:242-261)
        self.transfer_function.copy_(torch.from_numpy(tex), non_blocking=False)
        # acceleration tables of the texture; the separable-product claim made with the uniform is checked on the device
        self.ctx.transfer_function_tables(_ptr(self.transfer_function), self.get_transfer_function_uniform(), _ptr(self.transfer_function_bits),
                                          _stream())

    def update_transfer_function_on_device(self):
        """update_transfer_function_texture() without the host: texture + tables built on the device on the current stream, no wait.
        Same state afterwards (VolumeRenderSubpass picks it up)."""
        self.ctx.transfer_function_texture_device(self.options, _ptr(self.transfer_function), _ptr(self.transfer_function_bits), _stream())

    def update_transfer_function(self, skipping_type, d_count=None):
        """VolumeRender::update_transfer_function (src/volume_render.cpp:392-445) as one enqueue on the current stream: texture + tables,
        the occupancy map and the transform of `skipping_type` (grows the map list like ComputeDistanceMap.compute); `d_count`: a device
        int64 tensor that receives the occupied-voxel count."""
        self.set_number_of_distance_maps(8 if skipping_type == abi.SKIP_ANISOTROPIC_DISTANCE else 1)
        self.ctx.update_transfer_function(self.options, _ptr(self.volume), _ptr(self._gradient_or_none()), self.extent, _ptr(self.transfer_function),
                                          _ptr(self.transfer_function_bits), [_ptr(m) for m in self.distance_maps], _ptr(self.distance_map_swap),
                                          self.map_extent, skipping_type, _ptr(d_count), _stream())

    def _gradient_or_none(self):
        return self.gradient if self.options.use_precomputed_gradient else None

    def _out(self, name, out, box):
        """the tensor that Volume.<name> writes the voxels of `box` (None: all) into: the caller's `out`, which must be a contiguous uint8
        tensor of the volume's shape on its device, or a new one: a copy of the volume where a box leaves voxels unwritten"""
        if out is None:
            return self.volume.clone() if box is not None else torch.empty_like(self.volume)
        if out.dtype != torch.uint8 or out.shape != self.volume.shape or not out.is_contiguous() or out.device != self.volume.device:
            raise ValueError("Volume.%s: `out` must be a contiguous uint8 tensor of shape %s on %s" % (name, tuple(self.volume.shape), self.volume.device))
        return out

    def _box_shape(self, box):
        """[depth, height, width] of what a call over `box` (an abi.Box; None: the whole volume) writes per voxel"""
        return tuple(self.volume.shape) if box is None else (box.depth, box.height, box.width)

    def _check_labels(self, name, labels, box):
        """`labels` of Volume.<name>: a contiguous uint32 (or int32) tensor of the shape of `box` on the volume's device"""
        shape = self._box_shape(box)
        if labels.dtype not in (torch.uint32, torch.int32) or tuple(labels.shape) != shape or not labels.is_contiguous() or labels.device != self.volume.device:
            raise ValueError("Volume.%s: `labels` must be a contiguous uint32 tensor of shape %s on %s" % (name, shape, self.volume.device))

    def _scratch(self, nbytes, rejected):
        """the scratch block of a call that needs `nbytes` (a *_scratch_bytes result; 0: ValueError(rejected)), 8-byte aligned"""
        if nbytes == 0:
            raise ValueError(rejected)
        return torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=self.device)

    def _max_map_args(self, name, use_max_map):
        """(max_map, map_extent) of Volume.<name>(use_max_map=...): the volume's max map, which must have been built, or (None, None)"""
        if not use_max_map:
            return None, None
        if self.max_map is None:
            raise RuntimeError("Volume.%s: use_max_map=True needs the volume's max map (call Volume.build_max_map first)" % name)
        return self.max_map, self.map_extent

    def build_cell_summary(self, box=None):
        """The per-cell summaries of the occupancy map (vkv_cell_summary) on the current stream: of every cell (box None), or of the cells
        that meet ``box`` (an abi.Box or ((x0, y0, z0), (width, height, depth))).  The (cells, 16) uint8 buffer is allocated at the first
        call and kept in ``cell_summary``; it is built from the gradient map when use_precomputed_gradient is set.  update_region() keeps
        it current by rebuilding it over the update's box grown by one voxel per side."""
        box = _as_box(box)
        if self.cell_summary is None:
            if box is not None:
                raise ValueError("Volume.build_cell_summary: build the whole summary (box=None) first")
            me = self.map_extent
            self.cell_summary = torch.empty((me.width * me.height * me.depth, abi.CELL_SUMMARY_BYTES), dtype=torch.uint8, device=self.device)
        self.ctx.cell_summary(_ptr(self.volume), _ptr(self._gradient_or_none()), self.extent, self.map_extent, box, _ptr(self.cell_summary), _stream())
        return self.cell_summary

    def build_max_map(self, box=None):
        """The max map of the volume (vkv_max_map) on the current stream: per occupancy cell the largest voxel of the cell grown by one voxel
        per side, for every cell (box None) or the cells whose grown box meets ``box`` (an abi.Box or ((x0, y0, z0), (width, height, depth))).
        The (map depth, height, width) uint8 buffer is allocated at the first call and kept in ``max_map``; update_region() keeps it current.
        VolumeRenderSubpass.draw_mip(skip=True) skips over it."""
        box = _as_box(box)
        if self.max_map is None:
            if box is not None:
                raise ValueError("Volume.build_max_map: build the whole map (box=None) first")
            me = self.map_extent
            self.max_map = torch.empty((me.depth, me.height, me.width), dtype=torch.uint8, device=self.device)
        self.ctx.max_map(_ptr(self.volume), self.extent, self.map_extent, box, _ptr(self.max_map), _stream())
        return self.max_map

    def _check_colors(self, name, colors):
        """`colors` of <name>: a contiguous one-dimensional uint32 (or int32) tensor on the volume's device, one word per label"""
        if colors.dtype not in (torch.uint32, torch.int32) or colors.dim() != 1 or not colors.is_contiguous() or colors.device != self.volume.device:
            raise ValueError("%s: `colors` must be a contiguous one-dimensional uint32 tensor on %s" % (name, self.volume.device))

    def build_label_visibility_map(self, labels, colors, box=None):
        """The skipping map of VolumeRenderSubpass.draw_labels (vkv_label_visibility_map) on the current stream: per occupancy cell 255
        where a voxel of the cell grown by one voxel per side carries a label that ``colors`` shows, else 0.  ``labels``: as returned by
        label_components() for the same ``box`` (any contiguous uint32 device tensor of the box's shape does); ``colors``: a uint32 device
        tensor, entry L - 1 the R | G << 8 | B << 16 | A << 24 word of label L, alpha 0 hides the label (labels.color_table makes one).
        The (map depth, height, width) uint8 buffer is allocated at the first call and kept in ``label_visibility_map``; it belongs to these
        labels and this table, so call again after either changes.  No host wait."""
        box = _as_box(box)
        self._check_labels("build_label_visibility_map", labels, box)
        self._check_colors("Volume.build_label_visibility_map", colors)
        if self.label_visibility_map is None:
            me = self.map_extent
            self.label_visibility_map = torch.empty((me.depth, me.height, me.width), dtype=torch.uint8, device=self.device)
        n = colors.numel()
        self.ctx.check(self.ctx.label_visibility_map_rc(_ptr(labels), self.extent, box, _ptr(colors) if n else None, n, self.map_extent,
                                                        _ptr(self.label_visibility_map), _stream()))
        return self.label_visibility_map

    def update_transfer_function_from_summary(self, skipping_type, d_count=None, histogram=None, d_unresolved=None):
        """update_transfer_function() with the occupancy map decided from the cell summaries (vkv_update_transfer_function_from_summary):
        same texture, tables and maps.  ``d_count`` (an int64 device tensor) receives the occupied-voxel count read off ``histogram``
        (a histogram() result built with the same gradient setting), which it then requires; ``d_unresolved`` (an int64 device tensor)
        receives the number of cells evaluated from their voxels.  Call build_cell_summary() first."""
        if self.cell_summary is None:
            raise RuntimeError("Volume.update_transfer_function_from_summary: no cell summary (call build_cell_summary first)")
        if d_count is not None and histogram is None:
            raise ValueError("Volume.update_transfer_function_from_summary: d_count needs the histogram")
        self.set_number_of_distance_maps(8 if skipping_type == abi.SKIP_ANISOTROPIC_DISTANCE else 1)
        self.ctx.update_transfer_function_from_summary(self.options, _ptr(self.volume), _ptr(self._gradient_or_none()), self.extent,
                                                       _ptr(self.transfer_function), _ptr(self.transfer_function_bits),
                                                       [_ptr(m) for m in self.distance_maps], _ptr(self.distance_map_swap), self.map_extent,
                                                       skipping_type, _ptr(d_count), _ptr(self.cell_summary), _ptr(histogram), _ptr(d_unresolved),
                                                       _stream())

    _DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.int8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3}  # VkvVoxelType
    _TORCH_DTYPES = {torch.uint8: 0, torch.int8: 1, torch.int16: 3}

    def update_region(self, origin_xyz, voxels_dhw, skipping_type, voxel_type=None, big_endian=False, normalisation_range=None):
        """Write new voxels into the box at ``origin_xyz`` and rebuild what they reach, as one enqueue on the current stream
        (vkv_update_volume_region): the gradient map, the packed image (if built), and the occupancy + distance maps of ``skipping_type``
        (if built; it names what the maps hold, as in ComputeDistanceMap.compute).  ``voxels_dhw``: a (depth, height, width) numpy array
        (staged through pinned memory) or CUDA tensor of raw elements of ``voxel_type`` (default: from the dtype; a uint16 file's raw bytes
        come as int16 / uint16 with voxel_type = VKV_VOXEL_UINT16), converted like the loader converts a file: byte order, then
        ``normalisation_range`` (default (0, 255): uint8 voxels are stored as they are).  Precondition: the derived buffers are up to date
        (ComputeGradientMap / pack / ComputeDistanceMap with the current options and transfer function texture).  A cell summary built with
        build_cell_summary() is rebuilt over the box grown by one voxel per side, clamped to the volume (vkv_cell_summary's maintenance rule); a max
        map built with build_max_map() is rebuilt over the box."""
        if torch.is_tensor(voxels_dhw):
            src = voxels_dhw.to(self.device).contiguous()
            vt = self._TORCH_DTYPES.get(src.dtype) if voxel_type is None else voxel_type
        else:
            arr = np.ascontiguousarray(voxels_dhw)
            vt = self._DTYPES.get(arr.dtype) if voxel_type is None else voxel_type
            pinned = torch.from_numpy(arr.view(np.uint8).reshape(-1)).pin_memory()
            src = torch.empty(pinned.numel(), dtype=torch.uint8, device=self.device)
            src.copy_(pinned, non_blocking=True)  # (the pinned block is not reused before the copy has run: torch's host allocator)
        if vt is None:
            raise ValueError("Volume.update_region: no voxel type for dtype %s (pass voxel_type)" % (voxels_dhw.dtype,))
        d, h, w = voxels_dhw.shape
        lo, hi = (0.0, 255.0) if normalisation_range is None else normalisation_range
        maps = None
        if self.distance_maps:
            n = 8 if skipping_type == abi.SKIP_ANISOTROPIC_DISTANCE else 1
            if len(self.distance_maps) < n:
                raise RuntimeError("Volume.update_region: the maps of skipping type %d have not been built" % skipping_type)
            maps = [_ptr(m) for m in self.distance_maps[:n]]
        x, y, z = origin_xyz
        self.ctx.update_volume_region(_ptr(src), vt, big_endian, float(lo), float(hi), abi.Box(x, y, z, w, h, d), _ptr(self.volume),
                                      _ptr(self._gradient_or_none()), _ptr(self.packed), self.extent, _ptr(self.transfer_function), self.get_transfer_function_uniform(), maps,
                                      _ptr(self.distance_map_swap), self.map_extent, skipping_type, _stream())
        src.record_stream(torch.cuda.current_stream())  # the source stays allocated until the update has read it
        if self.cell_summary is not None:  # the summary of every cell the grown box meets (the gradient changes one voxel around the box)
            e = self.extent
            x0, y0, z0 = max(x - 1, 0), max(y - 1, 0), max(z - 1, 0)
            x1, y1, z1 = min(x + w + 1, e.width), min(y + h + 1, e.height), min(z + d + 1, e.depth)
            self.build_cell_summary(abi.Box(x0, y0, z0, x1 - x0, y1 - y0, z1 - z0))
        if self.max_map is not None:  # vkv_max_map rebuilds every cell whose grown box meets the update's box
            self.build_max_map(abi.Box(x, y, z, w, h, d))

    _HISTOGRAM_MODES = (abi.HISTOGRAM_SET, abi.HISTOGRAM_ADD, abi.HISTOGRAM_SUBTRACT)

    def histogram(self, out=None, box=None, mode=abi.HISTOGRAM_SET):
        """Joint histogram of (gradient byte, intensity byte) on the current stream (vkv_volume_histogram): a (256, 256) int64 CUDA tensor
        of the uint64 bins, row = gradient byte, column = intensity byte (as the transfer-function texture).  Uses the gradient map when
        use_precomputed_gradient is set, else counts every voxel in row 0.  ``out``: a contiguous (256, 256) int64 tensor on this volume's
        device to write into (required for ADD / SUBTRACT); ``box``: an abi.Box, or ((x0, y0, z0), (width, height, depth)); None: the
        whole volume.  SUBTRACT wraps modulo 2^64, so a histogram kept with SUBTRACT / ADD across update_region() stays exact."""
        if mode not in self._HISTOGRAM_MODES:
            raise ValueError("Volume.histogram: unknown mode %r" % (mode,))
        if out is None:
            if mode != abi.HISTOGRAM_SET:
                raise ValueError("Volume.histogram: ADD and SUBTRACT need `out`")
            out = torch.empty((256, 256), dtype=torch.int64, device=self.device)
        elif out.dtype != torch.int64 or tuple(out.shape) != (256, 256) or not out.is_contiguous() or out.device != self.volume.device:
            raise ValueError("Volume.histogram: `out` must be a contiguous (256, 256) int64 tensor on %s" % (self.volume.device,))
        box = _as_box(box)
        self.ctx.volume_histogram(_ptr(self.volume), _ptr(self._gradient_or_none()), self.extent, box, mode, _ptr(out), _stream())
        return out

    _FILTER_KINDS = (abi.FILTER_BINOMIAL3, abi.FILTER_MEDIAN3)

    def filter(self, kind, passes=1, out=None, box=None):
        """The volume filtered over each voxel's clamp-to-edge 3x3x3 neighbourhood on the current stream (vkv_filter_volume): a uint8 tensor
        of the volume's shape.  ``kind``: abi.FILTER_BINOMIAL3 (weights (1, 2, 1)^3 / 64, one rounding) or abi.FILTER_MEDIAN3.  ``passes`` > 1
        applies the filter that many times, ping-ponging between ``out`` and one temporary buffer.  ``out``: a contiguous uint8 tensor of
        the volume's shape on its device that does not alias it.  ``box`` (an abi.Box, or ((x0, y0, z0), (width, height, depth))): only the
        box's voxels of ``out`` are written, which keeps a filtered copy current after update_region(); it needs ``out`` and passes == 1.
        ``self.volume`` and the derived buffers are not touched: loading the result as a volume is the caller's decision."""
        if kind not in self._FILTER_KINDS:
            raise ValueError("Volume.filter: unknown kind %r" % (kind,))
        if int(passes) != passes or passes < 1:
            raise ValueError("Volume.filter: passes must be a positive integer")
        if out is None and box is not None:
            raise ValueError("Volume.filter: a box needs `out` (the bytes outside the box are kept)")
        out = self._out("filter", out, box)
        if box is not None:
            if passes != 1:
                raise ValueError("Volume.filter: a box takes one pass")
            box = _as_box(box)
        tmp = torch.empty_like(self.volume) if passes > 1 else None
        src = self.volume
        for i in range(1, passes + 1):
            dst = out if (passes - i) % 2 == 0 else tmp
            self.ctx.filter_volume(_ptr(src), _ptr(dst), self.extent, box, kind, _stream())
            src = dst
        return out

    def _label_table_args(self, name, colors, use_visibility_map):
        """(n_colors, visibility map, map_extent) of Volume.<name>(colors=..., use_visibility_map=...): the checked table's length (0: none)
        and the volume's label visibility map, which must have been built from a table, or (None, None)"""
        n_colors = 0
        if colors is not None:
            self._check_colors("Volume.%s" % name, colors)
            n_colors = colors.numel()
            if n_colors == 0:  # (the C call reads a NULL table of 0 entries as "every label is visible", the opposite of an empty table)
                raise ValueError("Volume.%s: an empty colour table shows nothing; pass colors=None to show every label" % name)
        if not use_visibility_map:
            return n_colors, None, None
        if colors is None or self.label_visibility_map is None:
            raise RuntimeError("Volume.%s: use_visibility_map=True needs `colors` and the volume's label visibility map "
                               "(call Volume.build_label_visibility_map first)" % name)
        return n_colors, self.label_visibility_map, self.map_extent

    @staticmethod
    def _capacity_pair(name, capacity):
        """(vertices, triangles) of Volume.<name>(capacity=...) as ints, or None"""
        if capacity is None:
            return None
        cap_v, cap_t = capacity
        if int(cap_v) != cap_v or int(cap_t) != cap_t or cap_v < 0 or cap_t < 0 or cap_v > 0xffffffff:
            raise ValueError("Volume.%s: capacity must be (vertices, triangles), non-negative integers, vertices below 2^32" % name)
        return int(cap_v), int(cap_t)

    @staticmethod
    def _check_vertex_total(name, vertices):
        """the vertex count that a counting call of Volume.<name> read back must fit the 32-bit indices"""
        if vertices > 0xffffffff:
            raise ValueError("Volume.%s: %d vertices are past 32-bit indices; extract the surface box by box" % (name, vertices))

    def extract_isosurface(self, iso, box=None, use_max_map=False, capacity=None):
        """The isosurface of the volume at ``iso`` as triangles on the current stream (vkv_isosurface_mesh: marching tetrahedra in a defined
        order, voxel-index coordinates): returns ``(triangles, total)``, an [n, 3, 3] float32 device tensor and the surface's triangle count.
        ``capacity`` None: a counting call, ONE host read of the total, then the emit into a tensor of exactly that size; total is an int.
        With a capacity it is one call and no host read: n = capacity, the rows past min(total, capacity) are not written, and total is the
        call's two-element int64 device tensor (the total, the rows written).  ``box`` (an abi.Box, or ((x0, y0, z0), (width, height,
        depth))): only the cubes inside it.  ``use_max_map``: skip empty tiles through the volume's max map (build_max_map() first; the
        same bits).  vkvolume_amd.mesh turns the result into texture or model space, welds it and writes STL."""
        box = _as_box(box)
        max_map, map_extent = self._max_map_args("extract_isosurface", use_max_map)
        if capacity is not None and (int(capacity) != capacity or capacity < 0):
            raise ValueError("Volume.extract_isosurface: capacity must be a non-negative integer or None")
        scratch = self._scratch(lib.mesh_scratch_bytes(self.extent, box),
                                "Volume.extract_isosurface: the box is empty or outside the volume, or the volume is too large")
        counts = torch.empty((2,), dtype=torch.int64, device=self.device)

        def call(tri, n):
            self.ctx.isosurface_mesh(_ptr(self.volume), self.extent, box, iso, _ptr(max_map), map_extent, _ptr(scratch), _ptr(tri), n, _ptr(counts),
                                     _stream())

        if capacity is not None:
            tri = torch.empty((int(capacity), 3, 3), dtype=torch.float32, device=self.device)
            call(tri if capacity else None, int(capacity))
            return tri, counts
        call(None, 0)
        total = int(counts[0].item())
        tri = torch.empty((total, 3, 3), dtype=torch.float32, device=self.device)
        if total:
            call(tri, total)
        return tri, total

    def extract_label_mesh(self, labels, colors=None, iso=None, box=None, use_visibility_map=False, capacity=None):
        """The surfaces of the visible bodies of ``labels`` on the current stream (vkv_label_mesh: marching tetrahedra in
        extract_isosurface()'s order, every tetrahedron cut once per visible label it touches): returns ``(triangles, triangle_labels,
        total)``, an [n, 3, 3] float32 device tensor, the [n] torch.uint32 label of each triangle and the triangle count.  Two bodies that
        touch share bit-equal vertices, and each label's triangles are closed wherever the body does not touch a face of the box.
        ``labels``: as returned by label_components() or split_bodies() for the same ``box``.  ``colors``: a colour table as for
        build_label_visibility_map() (alpha 0 hides a label, and so does a label past the table); None: every non-zero label is visible.
        ``iso`` None: vertices at edge midpoints, and the volume is not read; else a vertex is interpolated where the volume crosses ``iso``
        between its two voxels, so that the labels of label_components(iso, 14) give extract_isosurface(iso)'s triangles bit for bit.
        ``use_visibility_map``: skip tiles through the volume's label visibility map (build_label_visibility_map() with the same labels,
        box and colors first; the same bits).  ``capacity`` None: a counting call, ONE host read of the total, then the emit into tensors of
        exactly that size; total is an int.  With a capacity it is one call and no host read: n = capacity, the rows past min(total,
        capacity) are not written, and total is the call's two-element int64 device tensor.  vkvolume_amd.mesh splits the result by label
        (split_by_label), measures the bodies (body_measures) and writes one coloured PLY (write_ply with face_colors)."""
        box = _as_box(box)
        self._check_labels("extract_label_mesh", labels, box)
        n_colors, vis, map_extent = self._label_table_args("extract_label_mesh", colors, use_visibility_map)
        if capacity is not None and (int(capacity) != capacity or capacity < 0):
            raise ValueError("Volume.extract_label_mesh: capacity must be a non-negative integer or None")
        scratch = self._scratch(label_tables.mesh_scratch_bytes(self.extent, box),
                                "Volume.extract_label_mesh: the box is empty or outside the volume, or it holds more than 2^32 - 1 voxels")
        counts = torch.empty((2,), dtype=torch.int64, device=self.device)

        def call(tri, tri_labels, n):
            self.ctx.check(self.ctx.label_mesh_rc(_ptr(labels), self.extent, box, _ptr(colors), n_colors, None if iso is None else _ptr(self.volume), 0.0 if iso is None else iso, _ptr(vis), map_extent,
                                                  _ptr(scratch), _ptr(tri), _ptr(tri_labels), n, _ptr(counts), _stream()))

        def outputs(n):
            return (torch.empty((n, 3, 3), dtype=torch.float32, device=self.device), torch.empty((n,), dtype=torch.uint32, device=self.device))

        if capacity is not None:
            tri, tri_labels = outputs(int(capacity))
            call(tri if capacity else None, tri_labels if capacity else None, int(capacity))
            return tri, tri_labels, counts
        call(None, None, 0)
        total = int(counts[0].item())
        tri, tri_labels = outputs(total)
        if total:
            call(tri, tri_labels, total)
        return tri, tri_labels, total

    def extract_label_mesh_indexed(self, labels, colors=None, iso=None, box=None, use_visibility_map=False, normals=False, vertex_labels=False,
                                   capacity=None):
        """The surfaces of extract_label_mesh() as an indexed mesh on the current stream (vkv_label_mesh_indexed): returns ``(vertices, faces,
        face_labels, normals, vertex_labels)``: [nv, 3] float32, [nt, 3] torch.uint32, [nt] torch.uint32 and, where asked for, [nv, 3] float32
        gradient normals of the volume (not normalised; they need ``iso``) and [nv, 2] torch.uint32 pairs of the shown labels on either side
        of each vertex (0: nothing, the free surface), else None.  One vertex per crossing edge: ``vertices[faces]`` is extract_label_mesh()'s
        triangle list bit for bit, and two bodies that touch name the same vertices on their interface.  ``labels``, ``colors``, ``iso``,
        ``box`` and ``use_visibility_map`` as for extract_label_mesh().  ``capacity`` None: a counting call, ONE host read of the four counts,
        then the emit into tensors of exactly those sizes.  ``capacity=(vertices, triangles)``: one call and no host read; the tensors have
        those sizes, the rows past the written counts are not written, and a sixth result is the call's int64 device tensor (triangles,
        triangles written, vertices, vertices written).  vkvolume_amd.mesh cuts one body out (body_submesh), orients the normals per
        triangle (oriented_corner_normals), measures what touches what (contact_areas) and writes PLY."""
        box = _as_box(box)
        self._check_labels("extract_label_mesh_indexed", labels, box)
        n_colors, vis, map_extent = self._label_table_args("extract_label_mesh_indexed", colors, use_visibility_map)
        if normals and iso is None:
            raise ValueError("Volume.extract_label_mesh_indexed: normals are the volume's gradient and need `iso`")
        capacity = self._capacity_pair("extract_label_mesh_indexed", capacity)
        scratch = self._scratch(label_tables.mesh_indexed_scratch_bytes(self.extent, box),
                                "Volume.extract_label_mesh_indexed: the box is empty or outside the volume, or it holds more than 2^32 - 1 voxels")
        counts = torch.empty((4,), dtype=torch.int64, device=self.device)

        def call(nv, nt):
            vertices = torch.empty((nv, 3), dtype=torch.float32, device=self.device)
            faces = torch.empty((nt, 3), dtype=torch.uint32, device=self.device)
            face_labels = torch.empty((nt,), dtype=torch.uint32, device=self.device)
            nrm = torch.empty((nv, 3), dtype=torch.float32, device=self.device) if normals else None
            pairs = torch.empty((nv, 2), dtype=torch.uint32, device=self.device) if vertex_labels else None
            self.ctx.check(self.ctx.label_mesh_indexed_rc(
                _ptr(labels), self.extent, box, _ptr(colors), n_colors, None if iso is None else _ptr(self.volume), 0.0 if iso is None else iso, _ptr(vis),
                map_extent, _ptr(scratch), _ptr(vertices) if nv else None, _ptr(nrm) if nv else None, _ptr(pairs) if nv else None, nv,
                _ptr(faces) if nt else None, _ptr(face_labels) if nt else None, nt, _ptr(counts), _stream()))
            return vertices, faces, face_labels, nrm, pairs

        if capacity is not None:
            return call(*capacity) + (counts,)
        call(0, 0)
        total = counts.cpu().tolist()
        self._check_vertex_total("extract_label_mesh_indexed", total[2])
        return call(total[2], total[0])

    def extract_isosurface_indexed(self, iso, box=None, use_max_map=False, normals=False, capacity=None):
        """The isosurface of extract_isosurface() as an indexed mesh on the current stream (vkv_isosurface_mesh_indexed): returns ``(vertices,
        faces, normals)``: [nv, 3] float32, [nt, 3] torch.uint32 and, with ``normals``, [nv, 3] float32 gradient normals (not normalised,
        pointing from the inside out), else None.  One vertex per crossing edge: ``vertices[faces]`` is extract_isosurface()'s triangle list
        bit for bit.  ``capacity`` None: a counting call, ONE host read of the four counts, then the emit into tensors of exactly those sizes.
        ``capacity=(vertices, triangles)``: one call and no host read; the tensors have those sizes, the rows past the written counts are not
        written, and a fourth result is the call's int64 device tensor (triangles, triangles written, vertices, vertices written).  ``box``
        and ``use_max_map`` as for extract_isosurface().  vkvolume_amd.mesh unindexes the result and writes PLY."""
        box = _as_box(box)
        max_map, map_extent = self._max_map_args("extract_isosurface_indexed", use_max_map)
        capacity = self._capacity_pair("extract_isosurface_indexed", capacity)
        scratch = self._scratch(lib.mesh_indexed_scratch_bytes(self.extent, box),
                                "Volume.extract_isosurface_indexed: the box is empty or outside the volume, or the volume is too large")
        counts = torch.empty((4,), dtype=torch.int64, device=self.device)

        def call(nv, nt):
            vertices = torch.empty((nv, 3), dtype=torch.float32, device=self.device)
            faces = torch.empty((nt, 3), dtype=torch.uint32, device=self.device)
            nrm = torch.empty((nv, 3), dtype=torch.float32, device=self.device) if normals else None
            self.ctx.isosurface_mesh_indexed(_ptr(self.volume), self.extent, box, iso, _ptr(max_map), map_extent, _ptr(scratch),
                                             _ptr(vertices) if nv else None, _ptr(nrm) if nv else None, nv, _ptr(faces) if nt else None, nt,
                                             _ptr(counts), _stream())
            return vertices, faces, nrm

        if capacity is not None:
            return call(*capacity) + (counts,)
        call(0, 0)
        total = counts.cpu().tolist()
        self._check_vertex_total("extract_isosurface_indexed", total[2])
        if total[0] == 0 and total[2] == 0:
            return (torch.empty((0, 3), dtype=torch.float32, device=self.device), torch.empty((0, 3), dtype=torch.uint32, device=self.device),
                    torch.empty((0, 3), dtype=torch.float32, device=self.device) if normals else None)
        return call(total[2], total[0])

    _CONNECTIVITIES = (abi.CONNECT_6, abi.CONNECT_14, abi.CONNECT_26)

    def label_components(self, iso, connectivity=6, box=None, sizes=True, use_max_map=False):
        """The connected components of the voxels with value >= ``iso`` (the mesh's inside rule) on the current stream
        (vkv_label_components): returns ``(labels, sizes, counts)``.  ``labels``: a torch.uint32 tensor of the box's shape [depth, height,
        width] (the volume's without a box), 0 for outside voxels and 1 .. K for the components in the order of their first voxel, the
        numbering of scipy.ndimage.label.  ``sizes``: a torch.uint32 tensor of K voxel counts, or None with ``sizes=False``.  ``counts``: the
        call's int64 device tensor (K, the sizes written, the inside voxels).  ``connectivity``: 6, 14 (the marching-tetrahedra edges: the
        bodies extract_isosurface() separates) or 26.  With ``sizes`` a counting call runs first and K is read back to size the tensor
        exactly: ONE host wait.  ``box`` and ``use_max_map`` as for extract_isosurface()."""
        if connectivity not in self._CONNECTIVITIES:
            raise ValueError("Volume.label_components: connectivity must be 6, 14 or 26")
        box = _as_box(box)
        max_map, map_extent = self._max_map_args("label_components", use_max_map)
        scratch = self._scratch(lib.components_scratch_bytes(self.extent, box),
                                "Volume.label_components: the box is empty or outside the volume, or it holds more than 2^32 - 1 voxels")
        counts = torch.empty((3,), dtype=torch.int64, device=self.device)
        labels = torch.empty(self._box_shape(box), dtype=torch.uint32, device=self.device)

        def call(d_sizes, n):
            self.ctx.label_components(_ptr(self.volume), self.extent, box, iso, connectivity, _ptr(max_map), map_extent, _ptr(scratch), _ptr(labels),
                                      _ptr(d_sizes), n, _ptr(counts), _stream())

        call(None, 0)
        if not sizes:
            return labels, None, counts
        k = int(counts[0].item())
        d_sizes = torch.empty((k,), dtype=torch.uint32, device=self.device)
        if k:
            call(d_sizes, k)
        return labels, d_sizes, counts

    def remove_islands(self, iso, min_voxels=None, keep_largest=False, connectivity=6, fill=0, out=None, box=None):
        """The volume without its small connected components at ``iso`` on the current stream (vkv_label_components, then
        vkv_select_components): a uint8 tensor of the volume's shape in which every inside voxel (value >= iso) of a component with fewer
        than ``min_voxels`` voxels holds ``fill``; everything else is the volume's byte.  ``keep_largest=True`` keeps only the largest
        component: the sizes are read back to find it, which is one more host wait, and min_voxels = max(sizes), so ties are all kept.
        Exactly one of ``min_voxels`` and ``keep_largest`` must be given.  ``fill`` should lie below iso (the default 0 does for every iso >
        0).  ``out``: a contiguous uint8 tensor of the volume's shape on its device (``out=self.volume`` works in place); without it a copy
        is made.  ``box``: only the box's voxels take part and are written; components are those of the box alone.  ``self.volume`` and the
        derived buffers are not touched unless ``out`` is the volume: loading the result is the caller's decision.  In place, a max map built
        with build_max_map() is rebuilt over the box on the same stream, without a host wait, and stays current; the gradient map, the packed
        image, the cell summary and the occupancy and distance maps are the caller's to re-derive."""
        if (min_voxels is None) == (not keep_largest):
            raise ValueError("Volume.remove_islands: give exactly one of min_voxels and keep_largest")
        if min_voxels is not None and (int(min_voxels) != min_voxels or min_voxels < 0):
            raise ValueError("Volume.remove_islands: min_voxels must be a non-negative integer")
        if int(fill) != fill or not 0 <= fill <= 255:
            raise ValueError("Volume.remove_islands: fill must be a byte")
        box = _as_box(box)
        out = self._out("remove_islands", out, box)
        labels, sizes, counts = self.label_components(iso, connectivity=connectivity, box=box)
        if keep_largest:
            min_voxels = int(sizes.to(torch.int64).max().item()) if sizes.numel() else 0
        self.ctx.select_components(_ptr(self.volume), _ptr(out), self.extent, box, _ptr(labels), _ptr(sizes) if sizes.numel() else None, _ptr(counts),
                                   int(min_voxels), 0xffffffffffffffff, int(fill), _stream())
        self._written_in_place(out, box)
        return out

    def _written_in_place(self, out, box):
        """after a call that wrote the voxels of `box` (an abi.Box; None: all) into `out`: where `out` is the volume's own storage, the max
        map (if built) is rebuilt over the box on the current stream, as update_region() does; no host wait"""
        if self.max_map is not None and out.untyped_storage().data_ptr() == self.volume.untyped_storage().data_ptr():
            self.build_max_map(box)

    def component_stats(self, labels, counts, box=None, values=True, capacity=None):
        """The measurements of the labelled components on the current stream (vkv_component_stats): a ComponentStats over the device records
        of the labels 1 .. K.  ``labels``, ``counts``: as returned by label_components() for the same ``box``; any contiguous uint32 (or
        int32) device tensor of the box's shape [depth, height, width] with values 0 .. counts[0] does as well.  ``values=False`` measures
        geometry only: the volume is not read and the four value fields are 0.  ``capacity``: the number of records; None reads K from
        ``counts``, which is ONE host wait; with a number there is none, the labels above it are ignored, and records beyond
        min(K, capacity) are not written: they hold whatever the allocation held."""
        box = _as_box(box)
        self._check_labels("component_stats", labels, box)
        k = int(counts[0].item()) if capacity is None else int(capacity)
        raw = torch.empty((k, abi.COMPONENT_STATS_BYTES), dtype=torch.uint8, device=self.device)
        self.ctx.component_stats(_ptr(self.volume) if values else None, self.extent, box, _ptr(labels), _ptr(counts), _ptr(raw) if k else None, k, _stream())
        return ComponentStats(raw)

    def select_components(self, labels, keep, fill=0, out=None, box=None):
        """The volume without the components that a table rejects, on the current stream (vkv_select_components_by_table): a uint8 tensor of
        the volume's shape in which every voxel of the box whose label L (``labels``: as for component_stats()) has ``keep[L - 1]`` false
        holds ``fill``; everything else is the volume's byte, labels beyond the table included.  ``keep``: a bool or uint8 device tensor,
        one element per label, e.g. a comparison of ComponentStats views.  ``out``, ``box`` and what happens in place: as for
        remove_islands().  No host wait."""
        if int(fill) != fill or not 0 <= fill <= 255:
            raise ValueError("Volume.select_components: fill must be a byte")
        box = _as_box(box)
        self._check_labels("select_components", labels, box)
        if keep.dtype not in (torch.bool, torch.uint8) or keep.dim() != 1 or not keep.is_contiguous() or keep.device != self.volume.device:
            raise ValueError("Volume.select_components: `keep` must be a contiguous one-dimensional bool or uint8 tensor on %s" % (self.volume.device,))
        out = self._out("select_components", out, box)
        n = keep.numel()
        self.ctx.select_components_by_table(_ptr(self.volume), _ptr(out), self.extent, box, _ptr(labels), _ptr(keep) if n else None, n, int(fill), _stream())
        self._written_in_place(out, box)
        return out

    def clear_border(self, iso, connectivity=6, fill=0, out=None, box=None):
        """The volume without the components at ``iso`` that touch a face of the box (the whole volume without one): bodies that the scan
        cuts (skimage.segmentation.clear_border of the labels).  label_components(), component_stats(values=False), the keep table by
        torch on the device, select_components(): a component is kept when its bounding box touches no face of the box.  K is read back once
        to size the records: ONE host wait.  ``connectivity``, ``fill``, ``out``, ``box`` and what happens in place: as for
        remove_islands()."""
        box = _as_box(box)
        labels, _, counts = self.label_components(iso, connectivity=connectivity, box=box, sizes=False)
        stats = self.component_stats(labels, counts, box=box, values=False)
        b = abi.Box(0, 0, 0, *self.extent.as_tuple()) if box is None else box
        lo = torch.tensor([b.x0, b.y0, b.z0], dtype=torch.int64, device=self.device)
        hi = lo + torch.tensor([b.width - 1, b.height - 1, b.depth - 1], dtype=torch.int64, device=self.device)
        keep = ((stats.bbox_min > lo) & (stats.bbox_max < hi)).all(dim=1)
        return self.select_components(labels, keep, fill=fill, out=out, box=box)

    _DISTANCE_TARGETS = {"inside": abi.DISTANCE_TO_INSIDE, "outside": abi.DISTANCE_TO_OUTSIDE}

    def _distance_transform(self, src, iso, target, limit, box, weights=None):
        """vkv_distance_transform (weights None) or vkv_distance_transform_weighted (a checked triple) of the uint8 tensor `src` (the volume's
        shape) on the current stream; box: an abi.Box or None"""
        scratch = self._scratch(lib.distance_transform_scratch_bytes(self.extent, box),
                                "Volume.distance_transform: the box is empty or outside the volume, or it holds more than 2^32 - 1 voxels or an axis above 32768")
        dist2 = torch.empty(self._box_shape(box), dtype=torch.uint32, device=self.device)
        if weights is None:
            self.ctx.distance_transform(_ptr(src), self.extent, box, iso, target, limit, _ptr(scratch), _ptr(dist2), _stream())
        else:
            self.ctx.check(self.ctx.distance_transform_weighted_rc(_ptr(src), self.extent, box, iso, target, weights, limit, _ptr(scratch), _ptr(dist2),
                                                                   _stream()))
        return dist2

    @staticmethod
    def _as_weights(name, weights):
        """None, or the triple (wx, wy, wz) of positive integers below 2^32 as ints"""
        if weights is None:
            return None
        try:
            w = tuple(weights)
            ok = len(w) == 3 and all(int(a) == a and 1 <= a <= 0xffffffff for a in w)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("Volume.%s: weights must be None or three positive integers (x, y, z)" % name)
        return tuple(int(a) for a in w)

    def distance_transform(self, iso, to="inside", limit=None, box=None, weights=None):
        """The exact squared Euclidean distance transform on the current stream (vkv_distance_transform): a torch.uint32 tensor of the box's
        shape [depth, height, width] (the volume's without a box) that holds, per voxel, the squared distance in voxel units to the nearest
        voxel with value >= ``iso`` (``to="inside"``; the mesh's inside rule) or below it (``to="outside"``), 0 on such a voxel.  ``limit``:
        values are capped at it (cheaper: the work grows with the distance found); None: unlimited, and 0xffffffff everywhere where the box
        holds no such voxel.  Only the box's voxels exist: nothing beyond it counts as inside or outside.  No host wait.
        ``weights``: None, or three positive integers (x, y, z) for voxels that are not cubes (vkv_distance_transform_weighted; see
        spacing_weights()): the values are then (wx dx)^2 + (wy dy)^2 + (wz dz)^2, and ``limit`` is in those units.  Weights whose largest
        possible value in the box exceeds 0xfffffffe raise VkvError.  The weighted call's cost does not grow with the distance found; None
        stays on vkv_distance_transform, which is the faster one at small limits and wherever targets are dense: measured on the 1024 x 1024
        x 795 bench volume to the inside, the crossover lies between limits 10 (11.5 against 13.0 ms) and 101 (21.0 against 16.2 ms), and
        unlimited it is 207 against 36 ms (profiles/distance_weighted_times.txt); pass (1, 1, 1) to get the same values from the other call."""
        if to not in self._DISTANCE_TARGETS:
            raise ValueError("Volume.distance_transform: `to` must be 'inside' or 'outside'")
        if limit is not None and (int(limit) != limit or not 1 <= limit <= abi.DISTANCE_NONE):
            raise ValueError("Volume.distance_transform: limit must be an integer in 1 .. 0xffffffff or None")
        box = _as_box(box)
        return self._distance_transform(self.volume, iso, self._DISTANCE_TARGETS[to], limit, box, self._as_weights("distance_transform", weights))

    @staticmethod
    def spacing_weights(voxel_size, max_weight=64, rel_tol=1e-3):
        """Integer weights for a voxel size (sx, sy, sz), e.g. VkvVolumeHeader.voxel_size: ``((wx, wy, wz), unit)`` with w_a * unit close to
        s_a, so that a squared distance d2 of a weighted call is sqrt(d2) * unit in the caller's length.  With s_min the smallest size, m = 1,
        2, ... in turn gives w_a = floor(m s_a / s_min + 0.5), until a w_a would exceed ``max_weight``; the first m whose largest relative error
        max_a |w_a s_min / m - s_a| / s_a is at most ``rel_tol`` is taken, else the m with the smallest error (the smaller m of equals);
        unit = s_min / m.  (0.5, 0.5, 1.25) gives ((2, 2, 5), 0.25).  Sizes that are not finite and positive, and sizes whose ratio
        exceeds ``max_weight`` (no m fits), raise ValueError."""
        try:
            sizes = tuple(float(s) for s in voxel_size)
        except (TypeError, ValueError):
            sizes = ()
        if len(sizes) != 3 or not all(np.isfinite(s) and s > 0 for s in sizes):
            raise ValueError("Volume.spacing_weights: voxel_size must be three finite positive numbers")
        if int(max_weight) != max_weight or max_weight < 1 or not rel_tol >= 0:
            raise ValueError("Volume.spacing_weights: max_weight must be a positive integer and rel_tol non-negative")
        s_min = min(sizes)
        best = None
        m = 1
        while True:
            w = tuple(int(np.floor(m * s / s_min + 0.5)) for s in sizes)
            if max(w) > max_weight:
                break
            err = max(abs(wa * s_min / m - s) / s for wa, s in zip(w, sizes))
            if best is None or err < best[0]:
                best = (err, w, m)
            if err <= rel_tol:
                break
            m += 1
        if best is None:        # m = 1 already exceeds max_weight: the ratio of the sizes is above it
            raise ValueError("Volume.spacing_weights: the sizes' ratio exceeds max_weight")
        return best[1], s_min / best[2]

    @staticmethod
    def ball_radius2(radius=None, radius2=None):
        """The squared radius of a morphology call: ``radius2`` itself, or floor(radius * radius) in doubles (so sqrt(2) gives 2); the ball
        holds the offsets with dx^2 + dy^2 + dz^2 <= radius2.  At least 1: radius2 = 1 is the 6-neighbourhood, 2 the 18, 3 the 26."""
        if (radius is None) == (radius2 is None):
            raise ValueError("give exactly one of radius and radius2")
        if radius2 is None:
            if not radius >= 0:
                raise ValueError("radius must be a non-negative number")
            r2 = int(np.floor(float(radius) * float(radius)))
        else:
            if int(radius2) != radius2:
                raise ValueError("radius2 must be an integer")
            r2 = int(radius2)
        if not 1 <= r2 <= abi.DISTANCE_NONE - 1:
            raise ValueError("the squared radius must lie in 1 .. 0xfffffffe")
        return r2

    def _morphology(self, name, steps, iso, radius, radius2, inside_fill, outside_fill, out, box, weights=None):
        """steps: "erode" / "dilate" in order; the first reads the volume, each further one the result before it (in place in `out`)"""
        r2 = self.ball_radius2(radius, radius2)
        for f in (inside_fill, outside_fill):
            if int(f) != f or not 0 <= f <= 255:
                raise ValueError("Volume.%s: inside_fill and outside_fill must be bytes" % name)
        weights = self._as_weights(name, weights)
        box = _as_box(box)
        out = self._out(name, out, box)
        src = self.volume
        for step in steps:
            erode = step == "erode"
            dist2 = self._distance_transform(src, iso, abi.DISTANCE_TO_OUTSIDE if erode else abi.DISTANCE_TO_INSIDE, r2 + 1, box, weights)
            self.ctx.select_by_distance(_ptr(src), _ptr(out), self.extent, box, _ptr(dist2), 1, r2, int(outside_fill if erode else inside_fill), _stream())
            src = out
        self._written_in_place(out, box)
        return out

    def erode(self, iso, radius=None, radius2=None, inside_fill=255, outside_fill=0, out=None, box=None, weights=None):
        """The volume eroded by a ball on the current stream (vkv_distance_transform to the outside with limit radius2 + 1, then
        vkv_select_by_distance): a uint8 tensor of the volume's shape in which every inside voxel (value >= ``iso``) within the ball of an
        outside voxel holds ``outside_fill``; everything else is the volume's byte.  Give ``radius`` (radius2 = floor(radius * radius)) or
        ``radius2``.  ``outside_fill`` should lie below iso and ``inside_fill`` at or above it (dilate(), open() and close() write it).
        ``out``: a contiguous uint8 tensor of the volume's shape on its device (``out=self.volume`` works in place); without it a copy is
        made.  ``box``: only the box's voxels exist, take part and are written; nothing beyond the box is outside, so the erosion does not
        eat at the box's faces (scipy's border_value=1).  ``self.volume`` is not touched unless ``out`` is the volume.  In place, a max map
        built with build_max_map() is rebuilt over the box after the last step, on the same stream and without a host wait, so
        extract_isosurface / label_components(use_max_map=True) and draw_mip / draw_iso / draw_slab(skip=True) see the new voxels; the gradient
        map, the packed image, the cell summary and the occupancy and distance maps are the caller's to re-derive.
        ``weights``: None, or three positive integers (x, y, z) as for distance_transform(): ``radius`` and ``radius2`` are then in weighted
        units, a step along axis a counting w_a, and the ball holds the offsets with (wx dx)^2 + (wy dy)^2 + (wz dz)^2 <= radius2: with
        spacing_weights() of the voxel size, a ball in the caller's length and not an ellipsoid."""
        return self._morphology("erode", ("erode",), iso, radius, radius2, inside_fill, outside_fill, out, box, weights)

    def dilate(self, iso, radius=None, radius2=None, inside_fill=255, outside_fill=0, out=None, box=None, weights=None):
        """The volume dilated by a ball: every outside voxel within the ball of an inside voxel holds ``inside_fill``; see erode()."""
        return self._morphology("dilate", ("dilate",), iso, radius, radius2, inside_fill, outside_fill, out, box, weights)

    def open(self, iso, radius=None, radius2=None, inside_fill=255, outside_fill=0, out=None, box=None, weights=None):
        """The opening by a ball: erode(), then dilate() of the result.  It cuts bridges and removes parts thinner than the ball, after which
        remove_islands() can drop what they held on by; see erode()."""
        return self._morphology("open", ("erode", "dilate"), iso, radius, radius2, inside_fill, outside_fill, out, box, weights)

    def close(self, iso, radius=None, radius2=None, inside_fill=255, outside_fill=0, out=None, box=None, weights=None):
        """The closing by a ball: dilate(), then erode() of the result.  It fills pores and cracks thinner than the ball; see erode()."""
        return self._morphology("close", ("dilate", "erode"), iso, radius, radius2, inside_fill, outside_fill, out, box, weights)

    def _nearest_target(self, src, iso, target, limit, box, weights, distance=False):
        """vkv_nearest_target of the uint8 tensor `src` (the volume's shape) on the current stream: (nearest, dist2 or None); box: an abi.Box or
        None, weights: a checked triple"""
        scratch = self._scratch(lib.distance_transform_scratch_bytes(self.extent, box),
                                "Volume.nearest_target: the box is empty or outside the volume, or it holds more than 2^32 - 1 voxels or an axis above 32768")
        nearest = torch.empty(self._box_shape(box), dtype=torch.uint32, device=self.device)
        dist2 = torch.empty(self._box_shape(box), dtype=torch.uint32, device=self.device) if distance else None
        self.ctx.check(self.ctx.nearest_target_rc(_ptr(src), self.extent, box, iso, target, weights, limit, _ptr(scratch), _ptr(nearest), _ptr(dist2), _stream()))
        return nearest, dist2

    def _propagate_labels(self, nearest, labels, box, mask, mask_iso):
        """vkv_propagate_labels on the current stream: a new uint32 tensor of the box's shape; mask: a uint8 tensor of the volume's shape or None"""
        out = torch.empty(self._box_shape(box), dtype=torch.uint32, device=self.device)
        self.ctx.check(self.ctx.propagate_labels_rc(_ptr(nearest), _ptr(labels), _ptr(out), self.extent, box, _ptr(mask), float(mask_iso), _stream()))
        return out

    def nearest_target(self, iso, to="inside", limit=None, box=None, weights=None, distance=False):
        """The nearest-target (feature) transform on the current stream (vkv_nearest_target): a torch.uint32 tensor of the box's shape [depth,
        height, width] (the volume's without a box) that holds, per voxel, the index of the nearest voxel with value >= ``iso``
        (``to="inside"``) or below it (``to="outside"``): the box-linear index (z' * height + y') * width + x' in box coordinates, which is the
        index into any flattened array of the box's shape, so ``values.flatten()[nearest.long()]`` gathers.  Among several nearest targets the
        smallest index is taken, so the result is unique; a target voxel's nearest target is itself.  abi.NEAREST_NONE (0xffffffff) where the
        box holds no target or the squared distance is >= ``limit`` (None: unlimited).  ``weights``: None means (1, 1, 1); else as for
        distance_transform(), and ``limit`` is in weighted units.  ``distance=True`` returns ``(nearest, dist2)``, dist2 being what
        distance_transform(iso, to, limit, box, weights) gives.  scipy.ndimage.distance_transform_edt(return_indices=True) with unique ties.
        No host wait."""
        if to not in self._DISTANCE_TARGETS:
            raise ValueError("Volume.nearest_target: `to` must be 'inside' or 'outside'")
        if limit is not None and (int(limit) != limit or not 1 <= limit <= abi.DISTANCE_NONE):
            raise ValueError("Volume.nearest_target: limit must be an integer in 1 .. 0xffffffff or None")
        weights = self._as_weights("nearest_target", weights) or (1, 1, 1)
        nearest, dist2 = self._nearest_target(self.volume, iso, self._DISTANCE_TARGETS[to], limit, _as_box(box), weights, distance)
        return (nearest, dist2) if distance else nearest

    def expand_labels(self, labels, iso, radius=None, radius2=None, box=None, weights=None, mask=None, mask_iso=None):
        """Labels grown into their surroundings on the current stream (vkv_nearest_target, then vkv_propagate_labels): a new torch.uint32
        tensor of the box's shape in which every voxel within the ball of an inside voxel (value >= ``iso``) holds the label of the NEAREST
        inside voxel (the smallest index of equals), and 0 elsewhere: skimage.segmentation.expand_labels with unique ties.  ``labels``: the
        labels of this volume's inside voxels at ``iso``, as label_components() returns them for the same ``box``.  ``radius`` / ``radius2``:
        as for erode() (the call's limit is radius2 + 1); neither: unlimited, the Voronoi regions of the components.  ``weights``: as for
        nearest_target().  ``mask``: an optional Volume of the same extent that confines the growth: voxels of it below ``mask_iso``
        (None: ``iso``) get 0.  No host wait."""
        box = _as_box(box)
        self._check_labels("expand_labels", labels, box)
        limit = None if radius is None and radius2 is None else self.ball_radius2(radius, radius2) + 1
        weights = self._as_weights("expand_labels", weights) or (1, 1, 1)
        if mask is not None and (mask.extent.as_tuple() != self.extent.as_tuple() or mask.volume.device != self.volume.device):
            raise ValueError("Volume.expand_labels: `mask` must be a Volume of the same extent on the same device")
        nearest, _ = self._nearest_target(self.volume, iso, abi.DISTANCE_TO_INSIDE, limit, box, weights)
        return self._propagate_labels(nearest, labels, box, None if mask is None else mask.volume, iso if mask_iso is None else mask_iso)

    def _geodesic_call(self, d_seeds, iso, steps, limit, box, rounds, resume, scratch, dist, labels, counts):
        self.ctx.check(self.ctx.geodesic_propagate_rc(_ptr(self.volume), self.extent, box, iso, d_seeds, steps, limit, rounds, resume, _ptr(scratch), _ptr(dist),
                                                      _ptr(labels), _ptr(counts), _stream()))

    def geodesic_propagate(self, seeds, iso, steps=None, limit=None, box=None, rounds=None, distance=True):
        """Geodesic distance and label propagation INSIDE the mask on the current stream (vkv_geodesic_propagate): ``(labels, dist, counts)``.
        ``seeds``: a contiguous uint32 (or int32) tensor of the box's shape [depth, height, width]; a non-zero value on an inside voxel
        (value >= ``iso``) makes it a seed with that label.  Paths run through inside voxels of the box only, a move to one of the 26
        neighbours costing ``steps[|dx| + 2 |dy| + 4 |dz| - 1]`` (0: no such move; None: the 3-4-5 chamfer, distances in thirds of a voxel;
        see geodesic.chamfer_steps()).  ``dist`` (torch.uint32, None with ``distance=False``): the least cost from a seed, abi.GEODESIC_NONE
        where no seed is reached at a cost below ``limit`` (None: unlimited) and on outside voxels; ``labels`` (torch.uint32): the label of
        the seed at that cost, the smallest of equals, 0 where not reached.  ``counts``: the call's int64 device tensor: 1 once the result is
        final, and the reached voxels.  ``seeds`` is not written.
        ``rounds``: an integer 1 .. abi.GEODESIC_MAX_ROUNDS makes exactly ONE call of that many rounds, without a host wait; the caller
        reads ``counts[0]``, and while it is 0 the outputs are upper bounds only (a path needs about one round per 8 voxels of its length).
        None: a call of 64 rounds, then resumed calls of 128, 256, ... rounds (at most abi.GEODESIC_MAX_ROUNDS each) until ``counts[0]``
        is 1, which is read on the host between the calls: this is THE ONE HOST WAIT of the segmentation chain."""
        box = _as_box(box)
        self._check_labels("geodesic_propagate", seeds, box)
        steps = geodesic.CHAMFER_345 if steps is None else tuple(int(c) for c in steps)
        if len(steps) != 7:
            raise ValueError("Volume.geodesic_propagate: steps must be seven integers")
        if limit is not None and (int(limit) != limit or not 1 <= limit <= abi.GEODESIC_NONE):
            raise ValueError("Volume.geodesic_propagate: limit must be an integer in 1 .. 0xffffffff or None")
        if rounds is not None and (int(rounds) != rounds or not 1 <= rounds <= abi.GEODESIC_MAX_ROUNDS):
            raise ValueError("Volume.geodesic_propagate: rounds must be an integer in 1 .. %d or None" % abi.GEODESIC_MAX_ROUNDS)
        scratch = self._scratch(geodesic.scratch_bytes(self.extent, box),
                                "Volume.geodesic_propagate: the box is empty or outside the volume, or it holds more than 2^32 - 1 voxels")
        labels = torch.empty(self._box_shape(box), dtype=torch.uint32, device=self.device)
        dist = torch.empty(self._box_shape(box), dtype=torch.uint32, device=self.device) if distance else None
        counts = torch.empty((2,), dtype=torch.int64, device=self.device)
        n = 64 if rounds is None else int(rounds)
        self._geodesic_call(_ptr(seeds), iso, steps, limit, box, n, False, scratch, dist, labels, counts)
        while rounds is None and int(counts[0].item()) == 0:        # the host wait
            n = min(2 * n, abi.GEODESIC_MAX_ROUNDS)
            self._geodesic_call(None, iso, steps, limit, box, n, True, scratch, dist, labels, counts)
        return labels, dist, counts

    def grow_from_points(self, points, iso, steps=None, limit=None, box=None, rounds=None, distance=True):
        """Seeded region growing with a reach limit (click to select): geodesic_propagate() from the voxels ``points``, a sequence of
        (x, y, z) in volume coordinates, point i carrying the label i + 1 (of equal points the first).  A point on an outside voxel seeds
        nothing; a point outside the box (or the volume) raises ValueError.  ``labels != 0`` is the part of the clicked bodies within
        ``limit`` (in units of ``steps``; None: the whole bodies) of a point, each voxel with the label of the point it is reached from
        most cheaply.  Everything else, the host wait of ``rounds=None`` included, as for geodesic_propagate()."""
        box = _as_box(box)
        d, h, w = self._box_shape(box)
        x0, y0, z0 = (box.x0, box.y0, box.z0) if box is not None else (0, 0, 0)
        first = {}
        for k, point in enumerate(points):
            x, y, z = (int(c) for c in point)
            if not (x0 <= x < x0 + w and y0 <= y < y0 + h and z0 <= z < z0 + d):
                raise ValueError("Volume.grow_from_points: point %d, %r, lies outside the box" % (k, (x, y, z)))
            first.setdefault(((z - z0) * h + (y - y0)) * w + (x - x0), k + 1)
        seeds = torch.zeros((d, h, w), dtype=torch.int32, device=self.device)
        if first:
            index = torch.tensor(sorted(first), dtype=torch.int64, device=self.device)
            seeds.view(-1)[index] = torch.tensor([first[i] for i in sorted(first)], dtype=torch.int32, device=self.device)
        return self.geodesic_propagate(seeds, iso, steps=steps, limit=limit, box=box, rounds=rounds, distance=distance)

    def split_bodies(self, iso, radius=None, radius2=None, connectivity=6, box=None, weights=None, metric="euclidean"):
        """Touching bodies split at full size, on the current stream: ``(labels, counts)``.  erode() by the ball (``radius`` / ``radius2`` /
        ``weights`` as there), label_components() of the eroded volume (``connectivity``), nearest_target() of the eroded volume, unlimited,
        and vkv_propagate_labels with this volume as the mask at ``iso``: every inside voxel of THIS volume gets the label of the nearest
        surviving core, 0 only where nothing survived anywhere in the box, and outside voxels get 0.  ``labels`` (torch.uint32, the box's
        shape, values 0 .. K) and ``counts`` (label_components()'s, K first) go to component_stats() and select_components() unchanged, which
        then measure and select the full-size bodies.  "Nearest" is EUCLIDEAN, not geodesic: a thin fragment that vanished whole takes the
        label of a core across a gap, and a bridge is divided by the perpendicular bisector of the cores' surfaces, not by its waist.  The
        volume is not touched.  No host wait: label_components() runs with sizes=False.
        ``metric="geodesic"`` closes that gap: the erosion and the cores as above, then geodesic_propagate() of the cores' labels through
        THIS volume's inside voxels, unlimited, with the 3-4-5 chamfer (with ``weights``: geodesic.chamfer_steps(weights)): every inside
        voxel gets the label of the core it reaches most cheaply through inside voxels (26-connected), the smallest label of equals, and
        a voxel that reaches no core, such as a fragment across a gap, gets 0.  That call waits on the host for its rounds to settle."""
        if metric not in ("euclidean", "geodesic"):
            raise ValueError("Volume.split_bodies: metric must be 'euclidean' or 'geodesic'")
        box = _as_box(box)
        weights = self._as_weights("split_bodies", weights)
        eroded = Volume(self.ctx, self.name + ".eroded", device=self.device)
        eroded.volume, eroded.extent = self.erode(iso, radius=radius, radius2=radius2, box=box, weights=weights), self.extent
        core, _, counts = eroded.label_components(iso, connectivity=connectivity, box=box, sizes=False)
        if metric == "geodesic":
            steps = geodesic.chamfer_steps(weights)[0]
            return self.geodesic_propagate(core, iso, steps=steps, box=box, distance=False)[0], counts
        nearest, _ = eroded._nearest_target(eroded.volume, iso, abi.DISTANCE_TO_INSIDE, None, box, weights or (1, 1, 1))
        return self._propagate_labels(nearest, core, box, self.volume, iso), counts

    def occupied_count_from_histogram(self, hist, d_count):
        """The occupied-voxel count of the current options' analytic transfer function read off ``hist`` (a histogram() result) into
        ``d_count`` (a one-element int64 CUDA tensor), on the current stream; equals vkv_occupied_voxel_count when the histogram was built
        with the gradient map or use_gradient is 0."""
        if hist.dtype != torch.int64 or hist.numel() != abi.HISTOGRAM_BINS or not hist.is_contiguous():
            raise ValueError("Volume.occupied_count_from_histogram: `hist` must be a contiguous int64 tensor of %d bins" % abi.HISTOGRAM_BINS)
        if d_count.dtype != torch.int64 or d_count.numel() < 1:
            raise ValueError("Volume.occupied_count_from_histogram: `d_count` must be an int64 tensor")
        self.ctx.histogram_occupied_count(_ptr(hist), self.get_transfer_function_uniform(), _ptr(d_count), _stream())
        return d_count

    def pack(self):
        """(Re)build the bricked sampling image from the linear volume (+ gradient map).  Call after the gradient map
        is computed — the counterpart of the driver's swizzle into an optimally tiled VkImage.  The packed image is a COPY:
        after writing new voxels, use update_region(), which rebuilds only the bricks (and gradient and map cells) the box reaches;
        after writing to ``volume`` / ``gradient`` in place by other means, call pack() again (load_* and ComputeGradientMap do it themselves)."""
        if self.options.use_precomputed_gradient and not self.gradient_valid:
            raise RuntimeError("Volume.pack: use_precomputed_gradient is set but no gradient map has been computed "
                               "(run ComputeGradientMap.compute first)")
        n = self.ctx.packed_volume_bytes(self.extent)
        if self.packed is None or self.packed.numel() != n:
            self.packed = torch.empty(n, dtype=torch.uint8, device=self.device)
        self.ctx.pack_volume(_ptr(self.volume), _ptr(self._gradient_or_none()), self.extent, _ptr(self.packed), _stream())


class ComputeGradientMap:
    def __init__(self, ctx):
        self.ctx = ctx

    def compute(self, volume, transfer_function_uniform):
        self.ctx.gradient_map(_ptr(volume.volume), _ptr(volume.gradient), volume.extent, transfer_function_uniform, _stream())
        volume.gradient_valid = True
        if volume.use_packed:
            volume.pack()


class ComputeDistanceMap:
    def __init__(self, ctx):
        self.ctx = ctx

    def compute(self, volume, transfer_function_uniform, skipping_type):
        n = 8 if skipping_type == abi.SKIP_ANISOTROPIC_DISTANCE else 1
        volume.set_number_of_distance_maps(n)
        self.ctx.compute_distance_map(_ptr(volume.volume), _ptr(volume._gradient_or_none()), _ptr(volume.transfer_function), transfer_function_uniform,
                                      volume.extent, [_ptr(m) for m in volume.distance_maps], _ptr(volume.distance_map_swap),
                                      volume.map_extent, skipping_type, _stream())


class VolumeRenderSubpass:
    """Offscreen counterpart of the reference subpass: ``draw`` renders one volume into caller-provided buffers."""

    Options = abi.RenderOptions

    def __init__(self, ctx, volume, options=None, image_size=(256, 256)):
        self.ctx, self.volume = ctx, volume
        self.options = options if options is not None else abi.RenderOptions()
        self.image_size = image_size

    def make_params(self, view, proj, tiles=None, uniforms=None):
        """``uniforms``: an already built (CameraUniform, RayCastUniform, RayGen) triple instead of vkv_build_uniforms' (tests)."""
        v = self.volume
        w, h = self.image_size
        cam, rc, rg = uniforms if uniforms is not None else lib.build_uniforms(
            view, proj, v.node_transform, v.image_transform, self.options.clip_distance, (w, h), v.extent, v.map_extent)
        p = abi.RenderParams()
        p.camera, p.ray_cast, p.ray_gen = cam, rc, rg
        p.transfer_function = v.get_transfer_function_uniform()
        p.options = self.options
        p.use_precomputed_gradient = v.options.use_precomputed_gradient
        p.image_width, p.image_height = w, h
        p.tiles = tiles if tiles is not None else abi.full_frame_tiles(w, h)
        p.volume_extent, p.map_extent = v.extent, v.map_extent
        return self.bind(p)

    def bind(self, params):
        """Copy ``params`` and point it at this volume's device buffers (what draw() binds at
        src/volume_render_subpass.cpp:263-284)."""
        v = self.volume
        p = abi.RenderParams.from_buffer_copy(params)
        p.d_volume = _ptr(v.volume)
        p.d_gradient = _ptr(v._gradient_or_none())
        p.d_transfer_function = _ptr(v.transfer_function)
        for i in range(8):
            p.d_distance_maps[i] = _ptr(v.distance_maps[i]) if i < len(v.distance_maps) else None
        if v.use_packed and v.packed is None:
            v.pack()  # no gradient pass ran (on-the-fly / no-gradient variants): pack the volume channel alone
        p.d_packed_volume = _ptr(v.packed) if v.use_packed else None
        p.d_transfer_function_bits = _ptr(v.transfer_function_bits) if v.use_packed else None
        return p

    @staticmethod
    def _bind_outputs(params, color, rgba8, counts, depth=None, in_depth=None, blend=False):
        """point ``params`` at the buffers a draw call writes (None: not written) and reads (in_depth)"""
        params.d_out_color, params.d_out_rgba8 = _ptr(color), _ptr(rgba8)
        params.d_out_counts, params.d_out_depth = _ptr(counts), _ptr(depth)
        params.d_in_depth, params.blend_over_target = _ptr(in_depth), 1 if blend else 0

    def _skip_map(self, name, skip):
        """the max map that <name>(skip=...) skips over, which must have been built; None without skip"""
        if not skip:
            return None
        if self.volume.max_map is None:
            raise RuntimeError("VolumeRenderSubpass.%s: skip=True needs the volume's max map (call Volume.build_max_map first)" % name)
        return self.volume.max_map

    def draw(self, params, color=None, rgba8=None, counts=None, depth=None, in_depth=None, blend=False):
        """``in_depth``: scene depth for options.depth_attachment; ``blend``: blend onto the contents of color / rgba8
        (the subpass's blend state) instead of overwriting them."""
        self._bind_outputs(params, color, rgba8, counts, depth, in_depth, blend)
        self.ctx.render(params, _stream())

    def draw_mip(self, params, threshold, window_max, color=None, rgba8=None, intensity=None, depth=None, counts=None, skip=True, in_depth=None):
        """Maximum-intensity projection (vkv_render_mip) of ``params``' rays into the given buffers: samples > ``threshold`` count, the grey
        level is (m - threshold) / (window_max - threshold) clamped to [0, 1].  ``skip``: jump over the cells of the volume's max map
        (build_max_map() first; the same bits as the dense path); False: filter every sample.  ``in_depth``: scene depth for
        options.depth_attachment."""
        max_map = self._skip_map("draw_mip", skip)
        self._bind_outputs(params, color, rgba8, counts, depth, in_depth)
        mip = abi.MipOptions(threshold=float(threshold), window_max=float(window_max), d_max_map=_ptr(max_map), d_out_intensity=_ptr(intensity),
                             flags=0)
        self.ctx.render_mip(params, mip, _stream())

    def draw_iso(self, params, iso, refine_steps=4, base_color=(1.0, 1.0, 1.0), ambient=0.1, diffuse=0.8, specular=0.3, shininess=32, color=None,
                 rgba8=None, depth=None, normal=None, counts=None, skip=True, in_depth=None):
        """Shaded isosurface (vkv_render_isosurface) of ``params``' rays into the given buffers: the first sample whose filtered intensity is
        >= ``iso``, refined by ``refine_steps`` bisection steps, lit by a headlight (``base_color`` times ambient + diffuse + specular with the
        integer exponent ``shininess``); ``normal``: 4 floats per pixel, the world-space unit normal facing the camera.  ``skip``: jump over the
        cells of the volume's max map (build_max_map() first; the same bits as the dense path); False: filter every sample up to the hit.
        ``in_depth``: scene depth for options.depth_attachment."""
        max_map = self._skip_map("draw_iso", skip)
        self._bind_outputs(params, color, rgba8, counts, depth, in_depth)
        opts = abi.IsoOptions(iso=float(iso), refine_steps=int(refine_steps), base_color=(C.c_float * 3)(*[float(c) for c in base_color]),
                              ambient=float(ambient), diffuse=float(diffuse), specular=float(specular), shininess=int(shininess),
                              d_max_map=_ptr(max_map), d_out_normal=_ptr(normal), flags=0)
        self.ctx.render_isosurface(params, opts, _stream())

    def draw_labels(self, params, labels, colors, box=None, refine_steps=4, shade=True, ambient=0.1, diffuse=0.8, specular=0.3, shininess=32,
                    color=None, rgba8=None, label=None, depth=None, normal=None, counts=None, skip=True, in_depth=None):
        """A label volume as a picture (vkv_render_labels) of ``params``' rays into the given buffers: the first sample whose nearest voxel
        carries a label that ``colors`` shows, refined by ``refine_steps`` bisection steps, in that label's colour.  ``labels``, ``colors``,
        ``box``: as for Volume.build_label_visibility_map().  ``shade``: light the colour by draw_iso's headlight on the volume's gradient
        at the hit (``normal`` then receives the normal); False: the table's colour as it is, and the volume is not read.  ``label``: a
        uint32 (or int32) tensor, one element per pixel: the label under the pixel, 0 where nothing is hit (the pick buffer).  ``skip``:
        jump over the cells of the volume's label visibility map (build_label_visibility_map() with the same labels, box and colors first;
        the same bits as the dense path); False: look every sample up.  ``in_depth``: scene depth for options.depth_attachment."""
        box = _as_box(box)
        self.volume._check_labels("draw_labels", labels, box)
        self.volume._check_colors("VolumeRenderSubpass.draw_labels", colors)
        vis = None
        if skip:
            vis = self.volume.label_visibility_map
            if vis is None:
                raise RuntimeError("VolumeRenderSubpass.draw_labels: skip=True needs the label visibility map "
                                   "(call Volume.build_label_visibility_map first)")
        self._bind_outputs(params, color, rgba8, counts, depth, in_depth)
        n = colors.numel()
        opts = abi.LabelRenderOptions(d_labels=_ptr(labels), box=None if box is None else C.pointer(box), d_colors=_ptr(colors) if n else None,
                                      table_entries=n, refine_steps=int(refine_steps), shade=1 if shade else 0, ambient=float(ambient),
                                      diffuse=float(diffuse), specular=float(specular), shininess=int(shininess), d_visibility_map=_ptr(vis),
                                      d_out_label=_ptr(label), d_out_normal=_ptr(normal), flags=0)
        self.ctx.check(self.ctx.render_labels_rc(params, opts, _stream()))

    def pick(self, params, labels, colors, x, y, box=None):
        """The label under pixel (x, y) of ``params``' frame and its depth: ``(label, depth)``, (0, 0.0) where the ray hits nothing visible.
        Renders the one 16x16 tile that holds the pixel through a rect schedule, dense and unshaded, with draw_labels' default refinement
        and without the scene depth (options.depth_attachment is ignored), and reads the pixel back: ONE host wait."""
        w, h = params.image_width, params.image_height
        if not (0 <= x < w and 0 <= y < h):
            raise ValueError("VolumeRenderSubpass.pick: pixel (%d, %d) outside the %dx%d frame" % (x, y, w, h))
        p = abi.RenderParams.from_buffer_copy(params)
        p.options.depth_attachment = 0
        p.tiles = abi.full_frame_tiles(w, h, compact=True, rect=abi.TileRect(x // 16, y // 16, 1, 1))
        dev = self.volume.device
        label = torch.empty((256,), dtype=torch.uint32, device=dev)
        depth = torch.empty((256,), dtype=torch.float32, device=dev)
        self.draw_labels(p, labels, colors, box=box, shade=False, label=label, depth=depth, skip=False)
        at = (y % 16) * 16 + x % 16
        both = torch.stack([label.view(torch.int32)[at].to(torch.float64), depth[at].to(torch.float64)]).cpu()
        return int(both[0].item()) & 0xffffffff, float(both[1].item())

    def draw_slab(self, params, plane, samples=1, mode=abi.SLAB_MAX, window=(0.0, 1.0), skip=True, color=None, rgba8=None, value=None, counts=None):
        """Oblique slice or thick slab (vkv_render_slab) into the given buffers.  ``plane``: (origin, du, dv, dn) in texture coordinates, or
        the dict camera.slab_plane returns (pass its ``samples`` as ``samples``); pixel (x, y), sample j lies at origin + x du + y dv + j dn.  ``mode``: abi.SLAB_MAX / SLAB_MIN / SLAB_MEAN over the samples inside the volume; ``window``:
        (window_min, window_max) of the grey level; ``value``: one float per pixel, the slab's value.  ``skip`` (SLAB_MAX only; ignored by
        the other modes): jump over the cells of the volume's max map (build_max_map() first; the same bits as the dense path).  Only the
        image size, schedule and extents of ``params`` are read: no camera is needed."""
        if isinstance(plane, dict):
            plane = (plane["origin"], plane["du"], plane["dv"], plane["dn"])
        max_map = self._skip_map("draw_slab", skip and mode == abi.SLAB_MAX)
        self._bind_outputs(params, color, rgba8, counts)
        vec = lambda a: (C.c_float * 3)(*[float(x) for x in a])  # noqa: E731
        origin, du, dv, dn = plane
        opts = abi.SlabOptions(origin=vec(origin), du=vec(du), dv=vec(dv), dn=vec(dn), samples=int(samples), mode=int(mode),
                               window_min=float(window[0]), window_max=float(window[1]), d_max_map=_ptr(max_map), d_out_value=_ptr(value), flags=0)
        self.ctx.render_slab(params, opts, _stream())


def default_scene(volume, voxel_size=(1.0, 1.0, 1.0), axis_angle=(1.0, 0.0, 0.0, 0.0)):
    """image transform from the header fields + benchmark-mode node scale (src/load_volume.cpp:82-83,
    src/volume_render.cpp:224-238)."""
    e = volume.extent
    volume.set_image_transform(camera.image_transform(voxel_size, (e.width, e.height, e.depth), axis_angle))
    volume.node_transform = camera.benchmark_node_transform(volume.image_transform)
