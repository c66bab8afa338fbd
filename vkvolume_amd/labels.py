"""Host helpers of vkv_render_labels and vkv_label_visibility_map (include/vkvolume_amd.h): the colour table.  A table is a
numpy uint32 array with one word per label, entry L - 1 for label L: R in bits 0-7, G in bits 8-15, B in bits 16-23, A in bits 24-31.  Alpha
only switches a label on (not 0) or off (0).  Upload it with torch.from_numpy(table).to(device).  The table functions need no device and no
library; mesh_scratch_bytes() and mesh_indexed_scratch_bytes() ask the library (vkv_label_mesh, vkv_label_mesh_indexed)."""
import numpy as np

ALPHA = np.uint32(0xff000000)


def _mix(x):
    """a 32-bit integer hash (the finaliser of MurmurHash3), on uint64 so that the products do not overflow"""
    x = np.asarray(x, np.uint64) & np.uint64(0xffffffff)
    for shift, mul in ((16, 0x85ebca6b), (13, 0xc2b2ae35)):
        x ^= x >> np.uint64(shift)
        x = (x * np.uint64(mul)) & np.uint64(0xffffffff)
    return x ^ (x >> np.uint64(16))


def color_table(n_labels, seed=0, hidden=()):
    """A deterministic palette for the labels 1 .. n_labels: a numpy uint32 array of n_labels colour words with alpha 255, every channel in
    64 .. 255 (so no label is as dark as the background), the same for the same ``seed``; the labels listed in ``hidden`` get alpha 0."""
    n = int(n_labels)
    if n < 0:
        raise ValueError("labels.color_table: n_labels must not be negative")
    h = _mix(np.arange(1, n + 1, dtype=np.uint64) + (_mix(np.uint64(int(seed) & 0xffffffff) + np.uint64(0x9e3779b9)) << np.uint64(1)))
    r, g, b = (np.uint64(64) + ((h >> np.uint64(s)) & np.uint64(0xff)) * np.uint64(191) // np.uint64(255) for s in (0, 8, 16))
    table = (r | (g << np.uint64(8)) | (b << np.uint64(16))).astype(np.uint32) | ALPHA
    return set_visible(table, hidden, False)


def set_visible(table, labels, visible):
    """Switch the given labels (numbers 1 .. len(table)) of a colour table on (alpha 255) or off (alpha 0), in place; the colours stay.
    ``table``: a numpy uint32 array, or a torch uint32 / int32 tensor on any device (no host wait).  Returns the table.  After a change the
    visibility map of the table is stale: rebuild it (Volume.build_label_visibility_map)."""
    idx = np.asarray(list(labels), np.int64).reshape(-1)
    if idx.size and (idx.min() < 1 or idx.max() > len(table)):
        raise ValueError("labels.set_visible: labels must lie in 1 .. %d" % len(table))
    if isinstance(table, np.ndarray):
        if table.dtype != np.uint32 or table.ndim != 1:
            raise ValueError("labels.set_visible: the table must be a one-dimensional uint32 array")
        table[idx - 1] = (table[idx - 1] | ALPHA) if visible else (table[idx - 1] & ~ALPHA)
        return table
    import torch
    if table.dtype not in (torch.uint32, torch.int32) or table.dim() != 1:
        raise ValueError("labels.set_visible: the table must be a one-dimensional uint32 tensor")
    words = table.view(torch.int32)  # (alpha is the sign byte: 0xff000000 as int32 is -16777216)
    at = torch.from_numpy(idx - 1).to(table.device)
    words[at] = (words[at] | -16777216) if visible else (words[at] & 0x00ffffff)
    return table


def mesh_scratch_bytes(extent, box=None):
    """vkv_label_mesh_scratch_bytes: the scratch vkv_label_mesh needs for `box` (None: the whole volume) of `extent` (an abi.Extent3D): at
    least 16, a multiple of 8; 0 for an extent or box the call rejects (a box of more than 2^32 - 1 voxels included)"""
    from . import lib
    return lib.load().vkv_label_mesh_scratch_bytes(extent, box)


def mesh_indexed_scratch_bytes(extent, box=None):
    """vkv_label_mesh_indexed_scratch_bytes: the scratch vkv_label_mesh_indexed needs for `box` (None: the whole volume) of `extent` (an
    abi.Extent3D): at least 16, a multiple of 8; 0 for an extent or box the call rejects (a box of more than 2^32 - 1 voxels included)"""
    from . import lib
    return lib.load().vkv_label_mesh_indexed_scratch_bytes(extent, box)
