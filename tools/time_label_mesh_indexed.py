"""Cost of the indexed per-body mesh (vkv_label_mesh_indexed) next to the list it replaces (vkv_label_mesh) and next to the same output from
bytes (vkv_isosurface_mesh_indexed), in one run on the same buffers.

On the bench's C3 volume (1024x1024x795) with the labels of label_components(iso, 14) and the volume, vkv_label_mesh_indexed emits
vkv_isosurface_mesh_indexed's vertices, normals and indices (checked here, every byte).  Per scene:
  list count / full              vkv_label_mesh with the volume, NULL table: the list this call replaces
  iso indexed count / full       vkv_isosurface_mesh_indexed with normals: the same output from 1 B per voxel
  indexed count                  vkv_label_mesh_indexed, both capacities 0
  indexed full                   vertices, indices and triangle labels
  indexed full, normals+pairs    and normals and vertex labels
  ... , table                    each of the three through a colour table that shows every label
and, on C3, the labels of split_bodies(radius2=4) (bodies that touch: the list emits an interface's vertices once per body and triangle, the
indexed mesh once), at midpoints.  Each row: ms, the bytes the call WRITES into its outputs, and the time against the list's full call.
ms from device events (blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up
call of every variant; median [min .. max]).

    python tools/time_label_mesh_indexed.py [--iso 0.2] [--calls 5] [--repeats 7] [--out profiles/label_mesh_indexed_times.txt]
    python tools/time_label_mesh_indexed.py --rocprof [--out profiles/label_mesh_indexed_rocprof.txt]   the same run (one block of two calls) under
                                                    rocprofv3 --kernel-trace --stats, in a child process of its own, summarised per kernel
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, fmt, kernel_stats, ptr, run, stats_table, stream as st  # noqa: E402
from tools.scenes import scene_volume  # noqa: E402
from vkvolume_amd import labels as LB, lib  # noqa: E402


class Calls:
    """the three extractions of one volume with shared scratch"""

    def __init__(self, ctx, v):
        self.ctx, self.v, self.e = ctx, v, v.extent
        nbytes = max(LB.mesh_scratch_bytes(self.e), lib.mesh_indexed_scratch_bytes(self.e), LB.mesh_indexed_scratch_bytes(self.e))
        self.scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device="cuda")
        self.counts = torch.zeros((4,), dtype=torch.int64, device="cuda")

    def list(self, labels, table, vol, iso, tri, tl, capacity):
        self.ctx.check(self.ctx.label_mesh_rc(labels.data_ptr(), self.e, None, ptr(table), 0 if table is None else table.numel(), ptr(vol), iso, None, None,
                                              self.scratch.data_ptr(), ptr(tri), ptr(tl), capacity, self.counts.data_ptr(), st()))

    def iso_indexed(self, iso, vert, norm, cap_v, idx, cap_t):
        self.ctx.isosurface_mesh_indexed(self.v.volume.data_ptr(), self.e, None, iso, None, None, self.scratch.data_ptr(), ptr(vert), ptr(norm), cap_v,
                                         ptr(idx), cap_t, self.counts.data_ptr(), st())

    def indexed(self, labels, table, vol, iso, vert, norm, pair, cap_v, idx, tl, cap_t):
        self.ctx.check(self.ctx.label_mesh_indexed_rc(labels.data_ptr(), self.e, None, ptr(table), 0 if table is None else table.numel(), ptr(vol), iso, None,
                                                      None, self.scratch.data_ptr(), ptr(vert), ptr(norm), ptr(pair), cap_v, ptr(idx), ptr(tl), cap_t,
                                                      self.counts.data_ptr(), st()))

    def totals(self, fn):
        fn()
        return self.counts.cpu().tolist()


def report(out, kinds, runs, base):
    for k, (_, nbytes) in kinds.items():
        m = statistics.median(runs[k])
        out.append("  %-34s %s ms  writes %6.3f GB  (%5.2f x the list's full call)" % (k, fmt(runs[k]), nbytes / 1e9, m / base))


def buffers(nv, nt):
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    return (torch.empty((max(nv, 1), 3), **f32), torch.empty((max(nv, 1), 3), **f32), torch.empty((max(nv, 1), 2), **i32), torch.empty((max(nt, 1), 3), **i32),
            torch.empty((max(nt, 1),), **i32))


def measure(ctx, v, iso, name, calls, repeats, out, split=False):
    c = Calls(ctx, v)
    e = c.e
    n = e.width * e.height * e.depth
    vol = v.volume
    labels, _, counts = v.label_components(iso, connectivity=14, sizes=False)
    k = counts.cpu().tolist()[0]
    nt, _, nv, _ = c.totals(lambda: c.indexed(labels, None, vol, iso, None, None, None, 0, None, None, 0))
    assert c.totals(lambda: c.iso_indexed(iso, None, None, 0, None, 0)) == [nt, 0, nv, 0]
    assert c.totals(lambda: c.list(labels, None, vol, iso, None, None, 0))[0] == nt
    table = torch.from_numpy(LB.color_table(k, seed=1)).cuda()
    out.append("%s: volume %dx%dx%d (%.3f GB; labels %.3f GB) at iso %.3f: label_components(14): %d bodies; %d triangles, %d vertices (%.2f per triangle); "
               "scratch %.1f MB, of it %.1f MB crossing masks" % (name, e.width, e.height, e.depth, n / 1e9, 4 * n / 1e9, iso, k, nt, nv, nv / max(nt, 1),
                                                                  c.scratch.numel() * 8 / 1e6, ((e.width + 3) // 4 * 4) * e.height * e.depth / 1e6))
    tri = torch.empty((max(nt, 1), 3, 3), dtype=torch.float32, device="cuda")
    tl_list = torch.empty((max(nt, 1),), dtype=torch.int32, device="cuda")
    vert, norm, pair, idx, tl = buffers(nv, nt)
    vert2, norm2, _, idx2, _ = buffers(nv, nt)
    kinds = {
        "list count": (lambda: c.list(labels, None, vol, iso, None, None, 0), 0),
        "list full": (lambda: c.list(labels, None, vol, iso, tri, tl_list, nt), 40 * nt),
        "iso indexed count": (lambda: c.iso_indexed(iso, None, None, 0, None, 0), 0),
        "iso indexed full, normals": (lambda: c.iso_indexed(iso, vert2, norm2, nv, idx2, nt), 24 * nv + 12 * nt),
        "indexed count": (lambda: c.indexed(labels, None, vol, iso, None, None, None, 0, None, None, 0), 0),
        "indexed full": (lambda: c.indexed(labels, None, vol, iso, vert, None, None, nv, idx, tl, nt), 12 * nv + 16 * nt),
        "indexed full, normals+pairs": (lambda: c.indexed(labels, None, vol, iso, vert, norm, pair, nv, idx, tl, nt), 32 * nv + 16 * nt),
        "indexed count, table": (lambda: c.indexed(labels, table, vol, iso, None, None, None, 0, None, None, 0), 0),
        "indexed full, table": (lambda: c.indexed(labels, table, vol, iso, vert, None, None, nv, idx, tl, nt), 12 * nv + 16 * nt),
        "indexed full, normals+pairs, table": (lambda: c.indexed(labels, table, vol, iso, vert, norm, pair, nv, idx, tl, nt), 32 * nv + 16 * nt),
    }
    runs = alternate({name: fn for name, (fn, _) in kinds.items()}, calls, repeats)
    base = statistics.median(runs["list full"])
    report(out, kinds, runs, base)
    # the same output from bytes and from labels: every byte; and de-indexed, the list
    c.iso_indexed(iso, vert2, norm2, nv, idx2, nt)
    c.indexed(labels, None, vol, iso, vert, norm, pair, nv, idx, tl, nt)
    c.list(labels, None, vol, iso, tri, tl_list, nt)
    torch.cuda.synchronize()
    assert torch.equal(vert.view(torch.int32), vert2.view(torch.int32)) and torch.equal(norm.view(torch.int32), norm2.view(torch.int32)) and torch.equal(idx, idx2)
    assert torch.equal(tl, tl_list)
    del vert2, norm2, idx2
    torch.cuda.empty_cache()
    step = max(nt // 8, 1)
    for a in range(0, nt, step):
        b = min(a + step, nt)
        assert torch.equal(vert[idx[a:b].long()].view(torch.int32), tri[a:b].view(torch.int32))
    del tri, tl_list, vert, norm, pair, idx, tl, labels, table
    torch.cuda.empty_cache()
    if split:
        labels, _ = v.split_bodies(iso, radius2=4)
        bodies = int(labels.view(torch.int32).max())
        nt, _, nv, _ = c.totals(lambda: c.indexed(labels, None, None, 0.0, None, None, None, 0, None, None, 0))
        vert, _, pair, idx, tl = buffers(nv, nt)
        c.indexed(labels, None, None, 0.0, vert, None, pair, nv, idx, tl, nt)
        shared = int((pair.view(torch.int32) != 0).all(dim=1).sum())
        out.append("%s: split_bodies(radius2=4): %d bodies; %d triangles (the list: %d vertices), %d vertices (%.2f per triangle), %d of them (%.1f %%) shared "
                   "by two bodies" % (name, bodies, nt, 3 * nt, nv, nv / max(nt, 1), shared, 100.0 * shared / max(nv, 1)))
        tri = torch.empty((max(nt, 1), 3, 3), dtype=torch.float32, device="cuda")
        kinds = {
            "split list full, midpoints": (lambda: c.list(labels, None, None, 0.0, tri, tl, nt), 40 * nt),
            "split indexed count": (lambda: c.indexed(labels, None, None, 0.0, None, None, None, 0, None, None, 0), 0),
            "split indexed full, midpoints": (lambda: c.indexed(labels, None, None, 0.0, vert, None, None, nv, idx, tl, nt), 12 * nv + 16 * nt),
            "split indexed full, pairs": (lambda: c.indexed(labels, None, None, 0.0, vert, None, pair, nv, idx, tl, nt), 20 * nv + 16 * nt),
        }
        runs = alternate({name: fn for name, (fn, _) in kinds.items()}, calls, repeats)
        report(out, kinds, runs, statistics.median(runs["split list full, midpoints"]))
        del tri, vert, pair, idx, tl, labels
        torch.cuda.empty_cache()


def rocprof(args):
    rows = kernel_stats(__file__, ["--iso", str(args.iso), "--calls", "2", "--repeats", "1", "--no-salt", "--out", os.devnull], 900)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_label_mesh_indexed.py --iso %s --calls 2 --repeats 1 --no-salt` on one MI355X, a run of its own:" % args.iso,
            "# the kernels of vkv_label_mesh_indexed (k_lmeshi_*), vkv_label_mesh (k_lmesh_*) and vkv_isosurface_mesh_indexed (k_meshi_*) over all variants of",
            "# the c3 scene, ms per dispatch"] + stats_table(rows, ("k_meshi_", "k_lmesh_", "k_lmeshi_"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iso", type=float, default=0.2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-salt", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_label_mesh_indexed.py --iso %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (
            args.iso, args.calls, args.repeats)]
        v, _, _, _ = bench.build_scene(ctx, "c3")
        measure(ctx, v, args.iso, "c3", args.calls, args.repeats, lines, split=True)
        del v
        torch.cuda.empty_cache()
        if not args.no_salt:
            v, iso = scene_volume(ctx, "salt")
            measure(ctx, v, iso, "salt", args.calls, args.repeats, lines)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="label_mesh_indexed_times.txt", rocprof_name="label_mesh_indexed_rocprof.txt")


if __name__ == "__main__":
    main()
