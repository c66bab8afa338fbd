"""GPU: every box-of-voxels operation on a small box inside a volume of just over 2^32 bytes ("Above 2^32 bytes").

A box may hold at most 2^32 - 1 voxels, so on the 2048^3 volumes this library is built for these operations run on a box somewhere inside a
buffer whose byte offsets need 33 bits.  Here the box stays tiny (at most 70 x 21 x 19 voxels: 110 box-linear workgroups, several mesh tiles
in y and z, 81 geodesic tiles) and only the buffer around it is large; it is allocated and filled on the device and never copied to the
host.  The extents and boxes are tests/test_far_boxes_cpu.py's:
  A = 1000 x 1000 x 4400   the voxel at byte offset exactly 2^32 lies in the middle of a row of the "straddle" box, whose rows lie on both
                           sides of the boundary; the "far" box touches the three far faces;
  B = 2 x 65536 x 32800    z * H passes 2^31; the narrow-row kernels;
  C = 65536 x 33000 x 2    y * W and the plane pass 2^31.
A product formed in 32 bits, an int row index or a row load that goes wrong across the boundary lands inside the same allocation and reads or
writes the wrong voxels silently, so everything is judged by value: the reference is the suite's numpy statement on a host window around the
box (tests/test_far_boxes_cpu.py shows that the window is enough and that the surround fill alone gives another result), compared to the bit,
under the surround fills 0x00 and 0xFF.  The volume is a tests/helpers.py guarded() allocation made from its shape; after every call, on the
device: the box still holds its contents and no other byte of the payload differs from the fill, an output of the volume's or the map's
shape holds its pre-fill everywhere outside what the call is to write, and all guards are intact.  One large volume and at most one large
output are held at a time.  A test skips only where less than 12 GiB of device memory are free."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests import test_far_boxes_cpu as F
from tests.test_component_stats_cpu import DTYPE as STATS_DTYPE
from tests.test_distance_cpu import TO_INSIDE, TO_OUTSIDE
from tests.test_geodesic_cpu import CHAMFER
from vkvolume_amd import abi, geodesic, labels as LB, lib

pytestmark = pytest.mark.gpu
FILL = 0xA5          # pre-fill of every output, scratch included
ISO = F.ISO
GARBAGE = 0xBADC0FFEE0DDF00D
NEEDED = 12 << 30


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()
    _held.clear()
    torch.cuda.empty_cache()


def st():
    return torch.cuda.current_stream().cuda_stream


# ---- checks on the device -------------------------------------------------------------------------------------------------------------------
def guard_damage(h):
    """Guarded.check() without bringing the payload to the host: the indices of the guard bytes that no longer hold the fill"""
    bad = []
    for lo, hi in ((0, h.start), (h.stop, h.buf.numel())):
        part = h.buf[lo:hi].cpu().numpy()
        bad += [lo + int(i) for i in np.flatnonzero(part != h.fill)]
    return bad


def count_not(t, value):
    """the bytes of the contiguous uint8 tensor `t` that differ from `value`, a quarter GiB at a time"""
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    for part in t.reshape(-1).split(1 << 28):
        total += (part != value).sum()
    return int(total)


class Buffers:
    """the small guarded buffers of one call: outputs pre-filled with `prefill`, inputs copied in; check(): every guard intact, the inputs
    unchanged.  guard: the byte of the guards (None: the pre-fill's); offsets(name): by how many times its alignment the buffer `name` starts
    past a 256-byte boundary (None: 0).  After again() the same names give the same buffers once more, the outputs pre-filled anew and the
    scratch block as the call before left it."""

    def __init__(self, prefill=FILL, guard=None, offsets=None):
        self.prefill, self.guard, self.offsets = prefill, prefill if guard is None else guard, offsets or (lambda name: 0)
        self.handles, self.inputs, self.tail, self.made, self.second = [], [], None, {}, False

    def alloc(self, name, what, dtype=np.uint8, align=None):
        """(tensor, handle) of a guarded buffer that this object does not keep: `what` is a shape (pre-filled) or an array (copied in)"""
        item = what.dtype.itemsize if isinstance(what, np.ndarray) else np.dtype(dtype).itemsize
        if not isinstance(what, np.ndarray) and what[0] == 0:        # a capacity of 0: one element that has to keep its pre-fill (an empty tensor has no address)
            what = (1,) + tuple(what[1:])
        t, h = T.guarded(what, self.offsets(name) * (align or item), self.guard, "cuda", dtype=dtype)
        if not isinstance(what, np.ndarray) and self.prefill != self.guard:
            h.buf[h.start:h.stop].fill_(self.prefill)
        return t, h

    def out(self, name, shape, dtype=np.uint8, align=None):
        if self.second:
            t, h = self.made[name]
            if not name.startswith("d_scratch"):
                h.buf[h.start:h.stop].fill_(self.prefill)
            return t
        t, h = self.made[name] = self.alloc(name, tuple(shape), dtype, align)
        self.handles.append((name, h))
        return t

    def inp(self, name, array, align=None):
        if self.second:
            return self.made[name][0]
        a = np.ascontiguousarray(array)
        a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
        t, h = self.made[name] = self.alloc(name, a, align=align)
        self.handles.append((name, h))
        self.inputs.append((name, t, a))
        return t

    def scratch(self, nbytes, name="d_scratch"):
        """exactly nbytes of scratch: the allocation's payload is whole 8-byte words, the bytes past nbytes are not the call's to write"""
        t = self.out(name, ((nbytes + 7) // 8,), np.int64)
        self.tail = (t, nbytes)
        return t

    def again(self):
        self.second = True

    def check(self, what):
        for name, h in self.handles:
            bad = guard_damage(h)
            assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
        for name, t, a in self.inputs:
            assert np.array_equal(t.cpu().numpy(), a), "%s: the input %s changed" % (what, name)
        if self.tail is not None and self.tail[1] % 8:
            assert (self.tail[0].view(torch.uint8)[self.tail[1]:].cpu().numpy() == self.prefill).all(), "%s: bytes past the scratch block changed" % what


# ---- the large volume of a case ---------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, name, fill):
        _, ext, self.box, _ = F.CASE[name]
        self.extent = F.EXTENTS[ext]
        w, h, d = self.extent
        self.e, self.abox, self.fill = abi.Extent3D(w, h, d), abi.Box(*self.box), fill
        self.me = F.map_extent_of(self.extent)
        self.ame = abi.Extent3D(*self.me)
        self.contents, self.aux = F.case_inputs(name)
        self.shape = self.contents.shape
        self.d_vol, self.h_vol = T.guarded((d, h, w), 0, fill, "cuda")
        self.d_contents = torch.from_numpy(self.contents).cuda()
        self.region(self.d_vol).copy_(self.d_contents)
        self.nonfill = int((self.contents != fill).sum())
        self.whole_map = None
        torch.cuda.synchronize()

    def region(self, t):
        """the box of a tensor of the volume's shape"""
        x0, y0, z0, bw, bh, bd = self.box
        return t[z0:z0 + bd, y0:y0 + bh, x0:x0 + bw]

    def check_volume(self, what):
        bad = guard_damage(self.h_vol)
        assert not bad, "%s: d_volume: guard bytes %s changed (payload is bytes %d .. %d)" % (what, bad[:8], self.h_vol.start, self.h_vol.stop - 1)
        assert torch.equal(self.region(self.d_vol), self.d_contents), "%s: the volume's box changed" % what
        assert count_not(self.d_vol, self.fill) == self.nonfill, "%s: the volume changed outside the box" % what

    def max_map(self, ctx):
        """vkv_max_map of the whole volume, built once (test_far_box[...-max_map_whole] compares it)"""
        if self.whole_map is None:
            mw, mh, md = self.me
            self.whole_map = T.guarded((md, mh, mw), 0, FILL, "cuda")
            ctx.max_map(self.d_vol.data_ptr(), self.e, self.ame, None, self.whole_map[0].data_ptr(), st())
            torch.cuda.synchronize()
        return self.whole_map[0]


_held = {}        # at most one Scene


def scene(name, fill):
    if (name, fill) not in _held:
        _held.clear()
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info()[0]
        if free < NEEDED:
            pytest.skip("%.1f GiB of device memory free, %d needed" % (free / 2 ** 30, NEEDED >> 30))
        _held[(name, fill)] = Scene(name, fill)
    return _held[(name, fill)]


class SmallScene:
    """Scene's sibling for a volume small enough to come from the host (tests/test_gpu_box_ops_fuzz.py): it is its own window, with origin
    (0, 0, 0).  vol: the host array [d, h, w]; box: (x0, y0, z0, w, h, d) or None, the whole volume; me: the map extent (w, h, d) of the calls
    that take a map; B: the Buffers whose guard byte, pre-fill and offsets the volume and the map take"""

    def __init__(self, vol, box, aux, me, B):
        d, h, w = vol.shape
        self.extent, self.vol, self.aux, self.me, self.fill = (w, h, d), vol, aux, tuple(me), 0
        self.box = (0, 0, 0, w, h, d) if box is None else tuple(box)
        self.e, self.abox, self.ame = abi.Extent3D(w, h, d), None if box is None else abi.Box(*box), abi.Extent3D(*me)
        self.d_vol, self.h_vol = B.alloc("d_volume", vol)
        self.contents = np.ascontiguousarray(self.region(vol))
        self.d_contents = torch.from_numpy(self.contents).cuda()
        self.shape, self.whole_map, self.B = self.contents.shape, None, B

    region = Scene.region

    def check_volume(self, what):
        bad = guard_damage(self.h_vol)
        assert not bad, "%s: d_volume: guard bytes %s changed (payload is bytes %d .. %d)" % (what, bad[:8], self.h_vol.start, self.h_vol.stop - 1)
        assert np.array_equal(self.d_vol.cpu().numpy(), self.vol), "%s: the volume changed" % what

    def max_map(self, ctx):
        """vkv_max_map of the whole volume, built once on the device"""
        if self.whole_map is None:
            mw, mh, md = self.me
            self.whole_map = self.B.alloc("d_whole_map", (md, mh, mw))
            ctx.max_map(self.d_vol.data_ptr(), self.e, self.ame, None, self.whole_map[0].data_ptr(), st())
            torch.cuda.synchronize()
        return self.whole_map[0]


def cells_of(d_map, want):
    """the view of the map's cells that the reference names"""
    z, y, x = (int(v) for v in want["_at"])
    nz, ny, nx = want["cells"].shape[:3]
    assert z + nz <= d_map.shape[0] and y + ny <= d_map.shape[1] and x + nx <= d_map.shape[2]
    return d_map[z:z + nz, y:y + ny, x:x + nx]


def cells_and_rest(d_map, want, rest, what, restore=False):
    """the map's cells that the reference names, on the host; every other byte of the map holds `rest`"""
    sub = cells_of(d_map, want)
    got, keep = sub.cpu().numpy(), sub.clone()
    sub.fill_(rest)
    changed = count_not(d_map, rest)
    if restore:
        sub.copy_(keep)
    assert changed == 0, "%s: %d bytes of the map outside the cells of the call differ from %#x" % (what, changed, rest)
    return got


def volume_shaped(S, what, call, in_place=False, B=None):
    """the box of the output of call(d_dst), d_dst of the volume's shape: a second guarded allocation pre-filled with B's pre-fill, every byte
    of which outside the box must keep it; in place: the volume itself, whose box is put back"""
    if in_place:
        call(S.d_vol)
        torch.cuda.synchronize()
        got = S.region(S.d_vol).cpu().numpy()
        S.region(S.d_vol).copy_(S.d_contents)
        return got
    B = B or Buffers()
    w, h, d = S.extent
    d_dst, h_dst = B.alloc("d_dst", (d, h, w))
    try:
        call(d_dst)
        torch.cuda.synchronize()
        got = S.region(d_dst).cpu().numpy()
        bad = guard_damage(h_dst)
        assert not bad, "%s: d_dst: guard bytes %s changed" % (what, bad[:8])
        S.region(d_dst).fill_(B.prefill)
        changed = count_not(d_dst, B.prefill)
        assert changed == 0, "%s: %d bytes of d_dst outside the box changed" % (what, changed)
        return got
    finally:
        del d_dst, h_dst
        torch.cuda.empty_cache()


# ---- one call of each operation: f(ctx, S, want, B, what, **parameters) -> {name: whole output buffer} ----------------------------------------
# The parameters are the keywords of the references of tests/test_far_boxes_cpu.py, with the same defaults (the large cases' constants), and
# every call takes the whole drawn set of tests/box_ops_fuzz.py and ignores what it does not know (**_).  A capacity comes from the reference
# ("_cap0", "_cap1": what the parameters set), else it is the total + 5.
def run_max_map_box(ctx, S, want, B, what, **_):
    mw, mh, md = S.me
    d_map = B.out("d_max_map", (md, mh, mw))
    ctx.max_map(S.d_vol.data_ptr(), S.e, S.ame, S.abox, d_map.data_ptr(), st())
    torch.cuda.synchronize()
    return {"cells": cells_and_rest(d_map, want, B.prefill, what)}


def run_max_map_whole(ctx, S, want, B, what, **_):
    """every cell outside those around the box sees the surround fill alone"""
    return {"cells": cells_and_rest(S.max_map(ctx), want, S.fill, what, restore=True)}


def run_cell_summary(ctx, S, want, B, what, **_):
    mw, mh, md = S.me
    d_summary, h = B.alloc("d_summary", (md, mh, mw, abi.CELL_SUMMARY_BYTES), align=16)
    try:
        ctx.cell_summary(S.d_vol.data_ptr(), None, S.e, S.ame, S.abox, d_summary.data_ptr(), st())
        torch.cuda.synchronize()
        bad = guard_damage(h)
        assert not bad, "%s: d_summary: guard bytes %s changed" % (what, bad[:8])
        return {"cells": cells_and_rest(d_summary, want, B.prefill, what)}
    finally:
        del d_summary, h
        torch.cuda.empty_cache()


def run_histogram(ctx, S, want, B, what, mode=abi.HISTOGRAM_SET, **_):
    d_hist = B.out("d_histogram", (65536,), np.int64)
    ctx.volume_histogram(S.d_vol.data_ptr(), None, S.e, S.abox, mode, d_hist.data_ptr(), st())
    return {"hist": d_hist}


def run_filter(kind):
    def run(ctx, S, want, B, what, **_):
        return {"dst": volume_shaped(S, what, lambda d_dst: ctx.filter_volume(S.d_vol.data_ptr(), d_dst.data_ptr(), S.e, S.abox, kind, st()), B=B)}
    return run


def map_args(ctx, S, use_map):
    return (S.max_map(ctx).data_ptr(), S.ame) if use_map else (None, None)


def run_mesh(use_map):
    def run(ctx, S, want, B, what, iso=ISO, use_map=use_map, **_):
        cap = want.get("_cap0", len(want["triangles"]) + 5)
        nbytes = lib.mesh_scratch_bytes(S.e, S.abox)
        assert nbytes >= 16 and nbytes % 8 == 0, (what, nbytes)
        d_scratch, d_counts, d_tri = B.scratch(nbytes), B.out("d_counts", (2,), np.int64), B.out("d_triangles", (cap, 3, 3), np.float32)
        ctx.isosurface_mesh(S.d_vol.data_ptr(), S.e, S.abox, iso, *map_args(ctx, S, use_map), d_scratch.data_ptr(), d_tri.data_ptr(), cap, d_counts.data_ptr(),
                            st())
        return {"triangles": d_tri, "counts": d_counts}
    return run


def run_mesh_indexed(use_map):
    def run(ctx, S, want, B, what, iso=ISO, use_map=use_map, **_):
        cap_v, cap_t = want.get("_cap1", len(want["vertices"]) + 5), want.get("_cap0", len(want["indices"]) + 5)
        nbytes = lib.mesh_indexed_scratch_bytes(S.e, S.abox)
        assert nbytes >= 16 and nbytes % 8 == 0, (what, nbytes)
        d_scratch, d_counts = B.scratch(nbytes), B.out("d_counts", (4,), np.int64)
        d_vert, d_norm = B.out("d_vertices", (cap_v, 3), np.float32), B.out("d_normals", (cap_v, 3), np.float32)
        d_idx = B.out("d_indices", (cap_t, 3), np.int32)
        ctx.isosurface_mesh_indexed(S.d_vol.data_ptr(), S.e, S.abox, iso, *map_args(ctx, S, use_map), d_scratch.data_ptr(), d_vert.data_ptr(),
                                    d_norm.data_ptr() if cap_v else None, cap_v, d_idx.data_ptr(), cap_t, d_counts.data_ptr(), st())
        return {"vertices": d_vert, "normals": d_norm, "indices": d_idx, "counts": d_counts}
    return run


def run_components(connectivity, use_map):
    def run(ctx, S, want, B, what, iso=ISO, connectivity=connectivity, use_map=use_map, **_):
        cap = want.get("_cap0", int(want["counts"][0]) + 5)
        nbytes = lib.components_scratch_bytes(S.e, S.abox)
        assert nbytes >= 40 and nbytes % 8 == 0, (what, nbytes)
        d_scratch, d_counts = B.scratch(nbytes), B.out("d_counts", (3,), np.int64)
        d_labels, d_sizes = B.out("d_labels", S.shape, np.int32), B.out("d_sizes", (cap,), np.int32)
        ctx.label_components(S.d_vol.data_ptr(), S.e, S.abox, iso, connectivity, *map_args(ctx, S, use_map), d_scratch.data_ptr(), d_labels.data_ptr(),
                             d_sizes.data_ptr(), cap, d_counts.data_ptr(), st())
        return {"labels": d_labels, "sizes": d_sizes, "counts": d_counts}
    return run


def run_select_components(in_place):
    def run(ctx, S, want, B, what, lo=3, hi=F.EVERYTHING, fill=9, in_place=in_place, **_):
        a = S.aux
        d_labels, d_counts = B.inp("d_labels", a["labels"]), B.inp("d_counts", a["counts"])
        d_sizes = B.inp("d_sizes", a["sizes"] if len(a["sizes"]) else np.zeros(1, np.uint32))
        call = lambda d_dst: ctx.select_components(S.d_vol.data_ptr(), d_dst.data_ptr(), S.e, S.abox, d_labels.data_ptr(), d_sizes.data_ptr(),  # noqa: E731
                                                   d_counts.data_ptr(), lo, hi, fill, st())
        return {"dst": volume_shaped(S, what, call, in_place, B)}
    return run


def run_component_stats(ctx, S, want, B, what, **_):
    k = int(S.aux["counts"][0])
    cap = want.get("_cap0", k + 5)
    d_labels = B.inp("d_labels", S.aux["labels"])
    d_counts = B.inp("d_counts", np.array([k, GARBAGE, GARBAGE], np.uint64))
    d_stats = B.out("d_stats", ((cap + 3) * STATS_DTYPE.itemsize,), align=8)
    ctx.component_stats(S.d_vol.data_ptr(), S.e, S.abox, d_labels.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(), cap, st())
    return {"records": d_stats}


def run_select_by_table(ctx, S, want, B, what, fill=7, in_place=False, **_):
    d_labels, d_keep = B.inp("d_labels", S.aux["labels"]), B.inp("d_keep", S.aux["keep"])
    call = lambda d_dst: ctx.select_components_by_table(S.d_vol.data_ptr(), d_dst.data_ptr(), S.e, S.abox, d_labels.data_ptr(), d_keep.data_ptr(),  # noqa: E731
                                                        len(S.aux["keep"]), fill, st())
    return {"dst": volume_shaped(S, what, call, in_place, B)}


def distance_scratch(S, B, what):
    n = int(np.prod(S.shape))
    nbytes = lib.distance_transform_scratch_bytes(S.e, S.abox)
    assert nbytes == 4 * n + 8 * ((n + 63) // 64), (what, nbytes)
    return B.scratch(nbytes)


def accepted(ctx, rc, limit, what):
    """a limit of 0 is what the header rejects, before anything is enqueued; every other status is the context's error"""
    if limit == 0:
        assert rc == abi.VKV_E_INVALID_ARGUMENT, "%s: status %d for a limit of 0" % (what, rc)
    else:
        ctx.check(rc)


def run_distance(ctx, S, want, B, what, iso=ISO, calls=F.DISTANCE_CALLS, **_):
    d_scratch, got = distance_scratch(S, B, what), {}
    for target, limit in calls:
        key = "to %d limit %s" % (target, limit)
        got[key] = B.out("d_dist2 " + key, S.shape, np.int32)
        accepted(ctx, ctx.distance_transform_rc(S.d_vol.data_ptr(), S.e, S.abox, iso, target, limit, d_scratch.data_ptr(), got[key].data_ptr(), st()), limit, what)
    return got


def run_select_by_distance(ctx, S, want, B, what, lo=1, hi=9, fill=255, in_place=False, **_):
    d_dist = B.inp("d_dist2", S.aux["dist2"])
    call = lambda d_dst: ctx.select_by_distance(S.d_vol.data_ptr(), d_dst.data_ptr(), S.e, S.abox, d_dist.data_ptr(), lo, hi, fill, st())  # noqa: E731
    return {"dst": volume_shaped(S, what, call, in_place, B)}


def run_distance_weighted(ctx, S, want, B, what, iso=ISO, weights=F.WEIGHTS, limit=None, **_):
    d_scratch, got = distance_scratch(S, B, what), {}
    for target in (TO_INSIDE, TO_OUTSIDE):
        got["to %d" % target] = d_dist = B.out("d_dist2 to %d" % target, S.shape, np.int32)
        accepted(ctx, ctx.distance_transform_weighted_rc(S.d_vol.data_ptr(), S.e, S.abox, iso, target, weights, limit, d_scratch.data_ptr(), d_dist.data_ptr(),
                                                         st()), limit, what)
    return got


def run_nearest(ctx, S, want, B, what, iso=ISO, weights=F.WEIGHTS, target=TO_INSIDE, limit=None, **_):
    d_scratch, d_near, d_dist = distance_scratch(S, B, what), B.out("d_nearest", S.shape, np.int32), B.out("d_dist2", S.shape, np.int32)
    accepted(ctx, ctx.nearest_target_rc(S.d_vol.data_ptr(), S.e, S.abox, iso, target, weights, limit, d_scratch.data_ptr(), d_near.data_ptr(), d_dist.data_ptr(),
                                        st()), limit, what)
    return {"nearest": d_near, "dist2": d_dist}


def run_propagate(masked):
    def run(ctx, S, want, B, what, iso=ISO, **_):
        d_near, d_labels, d_out = B.inp("d_nearest", S.aux["nearest"]), B.inp("d_labels", S.aux["plabels"]), B.out("d_out", S.shape, np.int32)
        ctx.check(ctx.propagate_labels_rc(d_near.data_ptr(), d_labels.data_ptr(), d_out.data_ptr(), S.e, S.abox, S.d_vol.data_ptr() if masked else None,
                                          iso if masked else 0.0, st()))
        return {"out": d_out}
    return run


def run_geodesic(ctx, S, want, B, what, rounds=16, max_calls=40, iso=ISO, steps=CHAMFER, limit=None, **_):
    """`rounds` rounds from the seeds, then resumed calls of as many until d_counts[0] says that the state is the fixed point"""
    n = int(np.prod(S.shape))
    nbytes = geodesic.scratch_bytes(S.e, S.abox)
    assert nbytes == 8 * n + 32 + 8 * int(np.prod([-(-s // 8) for s in S.shape])), (what, nbytes)
    d_scratch, d_seeds, d_counts = B.scratch(nbytes), B.inp("d_seeds", S.aux["seeds"]), B.out("d_counts", (2,), np.int64)
    d_dist, d_labels = B.out("d_dist", S.shape, np.int32), B.out("d_labels", S.shape, np.int32)
    trace = []
    for call in range(max_calls):
        rc = ctx.geodesic_propagate_rc(S.d_vol.data_ptr(), S.e, S.abox, iso, None if call else d_seeds.data_ptr(), steps, limit, rounds, call > 0,
                                       d_scratch.data_ptr(), d_dist.data_ptr(), d_labels.data_ptr(), d_counts.data_ptr(), st())
        accepted(ctx, rc, limit, what)
        if limit == 0:
            return {"dist": d_dist, "labels": d_labels, "counts": d_counts}
        torch.cuda.synchronize()
        trace.append(int(d_counts[0].item()))
        assert trace[-1] in (0, 1), (what, trace)
        if trace[-1] == 1:
            break
    assert trace[-1] == 1, "%s: not settled after %d calls of %d rounds" % (what, max_calls, rounds)
    return {"dist": d_dist, "labels": d_labels, "counts": d_counts}


def run_visibility_map(ctx, S, want, B, what, **_):
    mw, mh, md = S.me
    d_labels, d_colors, d_map = B.inp("d_labels", S.aux["labels"]), B.inp("d_colors", S.aux["colors"]), B.out("d_map", (md, mh, mw))
    ctx.check(ctx.label_visibility_map_rc(d_labels.data_ptr(), S.e, S.abox, d_colors.data_ptr(), len(S.aux["colors"]), S.ame, d_map.data_ptr(), st()))
    torch.cuda.synchronize()
    return {"cells": cells_and_rest(d_map, want, 0, what)}


def label_table(ctx, S, B, table, use_map):
    """(d_labels, d_colors or None, table entries, d_visibility_map or None, its extent or None): with a table its colour words, and with a
    map vkv_label_visibility_map of the same labels, box and table, built on the device"""
    d_labels = B.inp("d_labels", S.aux["labels"])
    if not table:
        return d_labels, None, 0, None, None
    d_colors, n = B.inp("d_colors", S.aux["colors"]), len(S.aux["colors"])
    if not use_map:
        return d_labels, d_colors.data_ptr(), n, None, None
    mw, mh, md = S.me
    d_map = B.inp("d_visibility_map", np.full((md, mh, mw), B.prefill, np.uint8))
    if not B.second:
        ctx.check(ctx.label_visibility_map_rc(d_labels.data_ptr(), S.e, S.abox, d_colors.data_ptr(), n, S.ame, d_map.data_ptr(), st()))
        torch.cuda.synchronize()
        B.inputs[-1] = ("d_visibility_map", d_map, d_map.cpu().numpy())        # from here on an input that has to stay as it is
    return d_labels, d_colors.data_ptr(), n, d_map.data_ptr(), S.ame


def run_label_mesh(ctx, S, want, B, what, iso=ISO, table=False, use_map=False, **_):
    cap = want.get("_cap0", len(want["triangles"]) + 5)
    nbytes = LB.mesh_scratch_bytes(S.e, S.abox)
    assert nbytes >= 16 and nbytes % 8 == 0, (what, nbytes)
    d_labels, d_colors, entries, d_map, map_extent = label_table(ctx, S, B, table, use_map)
    d_scratch, d_counts = B.scratch(nbytes), B.out("d_counts", (2,), np.int64)
    d_tri, d_tl = B.out("d_triangles", (cap, 3, 3), np.float32), B.out("d_triangle_labels", (cap,), np.int32)
    ctx.check(ctx.label_mesh_rc(d_labels.data_ptr(), S.e, S.abox, d_colors, entries, S.d_vol.data_ptr(), iso, d_map, map_extent, d_scratch.data_ptr(),
                                d_tri.data_ptr(), d_tl.data_ptr(), cap, d_counts.data_ptr(), st()))
    return {"triangles": d_tri, "triangle_labels": d_tl, "counts": d_counts}


# name: (the reference of tests/test_far_boxes_cpu.py, the call)
OPERATIONS = {
    "max_map_box": ("max_map_box", run_max_map_box),
    "max_map_whole": ("max_map_whole", run_max_map_whole),
    "cell_summary": ("cell_summary", run_cell_summary),
    "histogram": ("histogram", run_histogram),
    "filter_binomial": ("filter_binomial", run_filter(abi.FILTER_BINOMIAL3)),
    "filter_median": ("filter_median", run_filter(abi.FILTER_MEDIAN3)),
    "mesh": ("mesh", run_mesh(False)),
    "mesh_max_map": ("mesh", run_mesh(True)),
    "mesh_indexed": ("mesh_indexed", run_mesh_indexed(False)),
    "mesh_indexed_max_map": ("mesh_indexed", run_mesh_indexed(True)),
    "components_6": ("components_6", run_components(6, False)),
    "components_6_max_map": ("components_6", run_components(6, True)),
    "components_26": ("components_26", run_components(26, False)),
    "components_26_max_map": ("components_26", run_components(26, True)),
    "select_components": ("select_components", run_select_components(False)),
    "select_components_in_place": ("select_components", run_select_components(True)),
    "component_stats": ("component_stats", run_component_stats),
    "select_by_table": ("select_by_table", run_select_by_table),
    "distance": ("distance", run_distance),
    "select_by_distance": ("select_by_distance", run_select_by_distance),
    "distance_weighted": ("distance_weighted", run_distance_weighted),
    "nearest": ("nearest", run_nearest),
    "propagate": ("propagate", run_propagate(False)),
    "propagate_masked": ("propagate_masked", run_propagate(True)),
    "geodesic": ("geodesic", run_geodesic),
    "visibility_map": ("visibility_map", run_visibility_map),
    "label_mesh": ("label_mesh", run_label_mesh),
}
assert {r for r, _ in OPERATIONS.values()} == set(F.REFERENCES)


def compare(got, want, what, fill=FILL):
    """every output buffer as a whole: the reference, then the pre-fill up to the buffer's end; to the bit"""
    for name, w in want.items():
        if name.startswith("_"):
            continue
        g = got[name]
        g = np.ascontiguousarray(g.cpu().numpy() if isinstance(g, torch.Tensor) else g)
        assert g.dtype.itemsize == w.dtype.itemsize and g.shape[1:] == w.shape[1:] and len(g) >= len(w), (what, name, g.dtype, g.shape, w.dtype, w.shape)
        expect = np.empty(g.shape, w.dtype)
        expect.view(np.uint8)[...] = fill
        expect[:len(w)] = w
        g = g.view(w.dtype)
        bad = g.view(np.uint8).reshape(g.shape + (-1,)) != expect.view(np.uint8).reshape(g.shape + (-1,))
        bad = bad.any(axis=-1)
        assert not bad.any(), "%s: %s: %d of %d elements differ, first at %s: got %s want %s" % (
            what, name, int(bad.sum()), bad.size, np.argwhere(bad)[:4].tolist(), g[bad][:4].tolist(), expect[bad][:4].tolist())


CALLS = [(name, fill, op) for name, _, _, _ in F.CASES for fill in F.FILLS for op in OPERATIONS]        # in this order: a volume is made once


@pytest.mark.parametrize("name,fill,op", CALLS, ids=["%s-fill_%02x-%s" % c for c in CALLS])
def test_far_box(ctx, name, fill, op):
    what = "%s, surround %#04x, %s" % (name, fill, op)
    S = scene(name, fill)
    reference, run = OPERATIONS[op]
    want = F.reference(name, reference, fill)
    B = Buffers()
    got = run(ctx, S, want, B, what)
    torch.cuda.synchronize()
    B.check(what)
    compare(got, want, what)
    S.check_volume(what)
    if S.whole_map is not None:
        bad = guard_damage(S.whole_map[1])
        assert not bad, "%s: the whole volume's max map: guard bytes %s changed" % (what, bad[:8])


def test_the_contents_are_those_of_the_distance_tests():
    from tests.test_gpu_distance import contents
    for name, _, box, seed in F.CASES:
        assert np.array_equal(F.case_inputs(name)[0], contents("random 0.5", (box[5], box[4], box[3]), seed=seed)), name
