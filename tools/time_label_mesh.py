"""Cost of per-body mesh extraction from labels (vkv_label_mesh) next to the isosurface mesh (vkv_isosurface_mesh) on the same volume.

The yardstick is vkv_isosurface_mesh on the bench's C3 volume (1024x1024x795) at the same iso in the same run: with the labels of
label_components(iso, 14) and the volume, vkv_label_mesh emits the identical triangle list (checked here, every byte), so the difference is
what reading 4 B per voxel instead of 1 and writing 4 B per triangle more costs.  Per iso, all in one run:
  isosurface count / full      vkv_isosurface_mesh: the counting call and the whole call at a capacity of the total
  label count / full           vkv_label_mesh with the volume, NULL table: the same list plus the labels
  label full, midpoints        without the volume (t = 0.5 everywhere; the volume is not read)
  label full, table            every label visible through a colour table (one lookup per distinct label of a non-uniform cube)
  label count / full, map      the same through vkv_label_visibility_map (block 4)
and once at the first iso the labels of split_bodies(radius2=4) (bodies that touch: interfaces are emitted twice, once per body), and the
salt-noise scene of tools/time_components.py (many one-voxel bodies), dense against the map.
Each row: ms, the algorithmic bytes (the input once per kernel that reads it: count reads it once, a full call twice; plus the outputs: 36 B
per triangle, and 4 B more with labels), GB/s of those bytes, and the time against the isosurface's full call of the same iso.
ms from device events (blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up
call of every variant; median [min .. max]).

    python tools/time_label_mesh.py [--isos 0.2,0.5] [--calls 5] [--repeats 7] [--out profiles/label_mesh_times.txt]
    python tools/time_label_mesh.py --rocprof [--out profiles/label_mesh_rocprof.txt]   the same run (one block of two calls) under rocprofv3
                                                                 --kernel-trace --stats, in a child process of its own, summarised per kernel
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
    """the two extractions of one volume with shared scratch and counts"""

    def __init__(self, ctx, v):
        self.ctx, self.v, self.e, self.me = ctx, v, v.extent, v.map_extent
        self.scratch = torch.empty((max(lib.mesh_scratch_bytes(self.e), LB.mesh_scratch_bytes(self.e)) // 8,), dtype=torch.int64, device="cuda")
        self.counts = torch.zeros((2,), dtype=torch.int64, device="cuda")

    def iso(self, iso, tri, capacity):
        self.ctx.isosurface_mesh(self.v.volume.data_ptr(), self.e, None, iso, None, None, self.scratch.data_ptr(), ptr(tri), capacity,
                                 self.counts.data_ptr(), st())

    def label(self, labels, table, vol, iso, vis, tri, tl, capacity):
        self.ctx.check(self.ctx.label_mesh_rc(labels.data_ptr(), self.e, None, ptr(table), 0 if table is None else table.numel(), ptr(vol), iso, ptr(vis),
                                              self.me if vis is not None else None, self.scratch.data_ptr(), ptr(tri), ptr(tl), capacity,
                                              self.counts.data_ptr(), st()))

    def total(self, fn):
        fn()
        return self.counts.cpu().tolist()[0]


def report(out, kinds, runs, base):
    for k, (_, nbytes) in kinds.items():
        m = statistics.median(runs[k])
        out.append("  %-30s %s ms  %6.3f GB  %7.1f GB/s  (%5.2f x the isosurface's full call)" % (k, fmt(runs[k]), nbytes / 1e9, nbytes / 1e9 / (m * 1e-3), m / base))


def measure_c3(ctx, isos, calls, repeats, out):
    v, _, _, _ = bench.build_scene(ctx, "c3")
    c = Calls(ctx, v)
    e, me = c.e, c.me
    n = e.width * e.height * e.depth
    vol = v.volume
    out.append("c3: volume %dx%dx%d (%.3f GB; labels %.3f GB), visibility map %dx%dx%d; scratch %.1f MB" % (
        e.width, e.height, e.depth, n / 1e9, 4 * n / 1e9, me.width, me.height, me.depth, c.scratch.numel() * 8 / 1e6))
    base = None
    for number, iso in enumerate(isos):
        labels, _, counts = v.label_components(iso, connectivity=14, sizes=False)
        k = counts.cpu().tolist()[0]
        nt = c.total(lambda: c.iso(iso, None, 0))
        assert c.total(lambda: c.label(labels, None, vol, iso, None, None, None, 0)) == nt
        table = torch.from_numpy(LB.color_table(k, seed=1)).cuda()
        vis = v.build_label_visibility_map(labels, table)
        out.append("iso %.2f: label_components(14): %d bodies; %d triangles (%.2f GB, labels %.2f GB); visibility map %.1f %% of cells empty" % (
            iso, k, nt, 36 * nt / 1e9, 4 * nt / 1e9, 100.0 * float((vis == 0).float().mean())))
        tri = torch.empty((max(nt, 1), 3, 3), dtype=torch.float32, device="cuda")
        tri2 = torch.empty((max(nt, 1), 3, 3), dtype=torch.float32, device="cuda")
        tl = torch.empty((max(nt, 1),), dtype=torch.int32, device="cuda")
        kinds = {
            "isosurface count": (lambda: c.iso(iso, None, 0), n),
            "isosurface full": (lambda: c.iso(iso, tri, nt), 2 * n + 36 * nt),
            "label count": (lambda: c.label(labels, None, vol, iso, None, None, None, 0), 4 * n),
            "label full": (lambda: c.label(labels, None, vol, iso, None, tri2, tl, nt), 8 * n + 40 * nt),
            "label full, midpoints": (lambda: c.label(labels, None, None, 0.0, None, tri2, tl, nt), 8 * n + 40 * nt),
            "label full, table": (lambda: c.label(labels, table, vol, iso, None, tri2, tl, nt), 8 * n + 40 * nt),
            "label count, map": (lambda: c.label(labels, table, vol, iso, vis, None, None, 0), 4 * n),
            "label full, map": (lambda: c.label(labels, table, vol, iso, vis, tri2, tl, nt), 8 * n + 40 * nt),
        }
        runs = alternate({name: fn for name, (fn, _) in kinds.items()}, calls, repeats)
        base = statistics.median(runs["isosurface full"])
        report(out, kinds, runs, base)
        # the two calls emit one list: every byte
        c.iso(iso, tri, nt)
        c.label(labels, None, vol, iso, None, tri2, tl, nt)
        torch.cuda.synchronize()
        assert c.counts.cpu().tolist() == [nt, nt] and torch.equal(tri.view(torch.int32), tri2.view(torch.int32))
        assert int(tl.min()) >= 1 and int(tl.max()) <= k
        del tri2
        if number == 0:
            split, _ = v.split_bodies(iso, radius2=4)
            ns = c.total(lambda: c.label(split, None, None, 0.0, None, None, None, 0))
            bodies = int(split.view(torch.int32).max())
            out.append("iso %.2f: split_bodies(radius2=4): %d bodies; %d triangles (%.2f x the isosurface's: an interface is emitted once per body)" % (
                iso, bodies, ns, ns / max(nt, 1)))
            tri2 = torch.empty((max(ns, 1), 3, 3), dtype=torch.float32, device="cuda")
            tl2 = torch.empty((max(ns, 1),), dtype=torch.int32, device="cuda")
            kinds = {
                "split count": (lambda: c.label(split, None, vol, iso, None, None, None, 0), 4 * n),
                "split full": (lambda: c.label(split, None, vol, iso, None, tri2, tl2, ns), 8 * n + 40 * ns),
                "split full, midpoints": (lambda: c.label(split, None, None, 0.0, None, tri2, tl2, ns), 8 * n + 40 * ns),
            }
            report(out, kinds, alternate({name: fn for name, (fn, _) in kinds.items()}, calls, repeats), base)
            del tri2, tl2, split
        del tri, tl, labels, table
        torch.cuda.empty_cache()


def measure_salt(ctx, calls, repeats, out):
    v, iso = scene_volume(ctx, "salt")
    c = Calls(ctx, v)
    e, me = c.e, c.me
    n = e.width * e.height * e.depth
    vol = v.volume
    labels, _, counts = v.label_components(iso, connectivity=14, sizes=False)
    k = counts.cpu().tolist()[0]
    nt = c.total(lambda: c.iso(iso, None, 0))
    table = torch.from_numpy(LB.color_table(k, seed=1, hidden=range(2, k + 1, 2))).cuda()
    vis = v.build_label_visibility_map(labels, table)
    nh = c.total(lambda: c.label(labels, table, vol, iso, None, None, None, 0))
    out.append("salt: volume %dx%dx%d at iso %.3f: %d bodies, %d triangles; every second body hidden: %d triangles, visibility map %.1f %% of cells empty" % (
        e.width, e.height, e.depth, iso, k, nt, nh, 100.0 * float((vis == 0).float().mean())))
    tri = torch.empty((max(nt, 1), 3, 3), dtype=torch.float32, device="cuda")
    tl = torch.empty((max(nt, 1),), dtype=torch.int32, device="cuda")
    kinds = {
        "isosurface count": (lambda: c.iso(iso, None, 0), n),
        "isosurface full": (lambda: c.iso(iso, tri, nt), 2 * n + 36 * nt),
        "label count": (lambda: c.label(labels, None, vol, iso, None, None, None, 0), 4 * n),
        "label full": (lambda: c.label(labels, None, vol, iso, None, tri, tl, nt), 8 * n + 40 * nt),
        "label count, half hidden": (lambda: c.label(labels, table, vol, iso, None, None, None, 0), 4 * n),
        "label full, half hidden": (lambda: c.label(labels, table, vol, iso, None, tri, tl, nh), 8 * n + 40 * nh),
        "label count, half hidden, map": (lambda: c.label(labels, table, vol, iso, vis, None, None, 0), 4 * n),
        "label full, half hidden, map": (lambda: c.label(labels, table, vol, iso, vis, tri, tl, nh), 8 * n + 40 * nh),
    }
    runs = alternate({name: fn for name, (fn, _) in kinds.items()}, calls, repeats)
    report(out, kinds, runs, statistics.median(runs["isosurface full"]))


def rocprof(args):
    rows = kernel_stats(__file__, ["--isos", args.isos, "--calls", "2", "--repeats", "1", "--no-salt", "--out", os.devnull], 900)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_label_mesh.py --isos %s --calls 2 --repeats 1 --no-salt` on one MI355X, a run of its own:" % args.isos,
            "# the kernels of vkv_label_mesh (k_lmesh_*) and of vkv_isosurface_mesh (k_mesh_*) over all variants and isos of the c3 scene, ms per dispatch"
            ] + stats_table(rows, ("k_mesh_", "k_lmesh_"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--isos", default="0.2,0.5")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-salt", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_label_mesh.py --isos %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (
            args.isos, args.calls, args.repeats)]
        measure_c3(ctx, [float(t) for t in args.isos.split(",")], args.calls, args.repeats, lines)
        if not args.no_salt:
            measure_salt(ctx, args.calls, args.repeats, lines)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="label_mesh_times.txt", rocprof_name="label_mesh_rocprof.txt")


if __name__ == "__main__":
    main()
