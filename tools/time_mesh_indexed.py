"""Cost of indexed isosurface extraction (vkv_isosurface_mesh_indexed) next to the triangle list (vkv_isosurface_mesh) on the bench's C3 volume.

C3 (1024x1024x795; bench.py's volume), per iso value, all in one run:
  list count / full            vkv_isosurface_mesh: the counting call and the whole call at a capacity of the total (36 B per triangle)
  indexed count                the counting call: both counts and both scans
  indexed full                 vertices + indices at capacities of the totals, no normals (12 B per vertex + 12 B per triangle)
  indexed full + normals       and the gradient normals (12 B per vertex more)
  indexed full + normals, map  the same through the max map (block 4)
  indexed vertices / indices   one list alone, the other capacity 0: where the full call's time goes
Each row: ms, the bytes the call writes to its outputs, GB/s of those bytes, and the time against the list's full call of the same run.
ms from device events (blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up
call of every variant; median [min .. max]).

    python tools/time_mesh_indexed.py [--isos 0.2,0.5] [--calls 5] [--repeats 7] [--out profiles/mesh_indexed_times.txt]
    python tools/time_mesh_indexed.py --rocprof [--out profiles/mesh_indexed_rocprof.txt]   the same run (one block of two calls) under rocprofv3
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
from vkvolume_amd import lib  # noqa: E402


def measure(ctx, isos, calls, repeats, out):
    v, _, _, _ = bench.build_scene(ctx, "c3")
    e, me = v.extent, v.map_extent
    n = e.width * e.height * e.depth
    vol = v.volume
    max_map = v.build_max_map()
    list_scratch = torch.empty((lib.mesh_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    scratch = torch.empty((lib.mesh_indexed_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    list_counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    counts = torch.zeros((4,), dtype=torch.int64, device="cuda")
    out.append("c3: volume %dx%dx%d (%.3f GB), max map %dx%dx%d; scratch: list %.1f MB, indexed %.1f MB" % (
        e.width, e.height, e.depth, n / 1e9, me.width, me.height, me.depth, list_scratch.numel() * 8 / 1e6, scratch.numel() * 8 / 1e6))

    def soup(iso, tri, capacity):
        ctx.isosurface_mesh(vol.data_ptr(), e, None, iso, None, None, list_scratch.data_ptr(), ptr(tri), capacity, list_counts.data_ptr(), st())

    def indexed(iso, skip, vert, norm, nv, idx, nt):
        ctx.isosurface_mesh_indexed(vol.data_ptr(), e, None, iso, max_map.data_ptr() if skip else None, me if skip else None, scratch.data_ptr(),
                                    ptr(vert), ptr(norm), nv, ptr(idx), nt, counts.data_ptr(), st())

    for iso in isos:
        indexed(iso, False, None, None, 0, None, 0)
        nt, _, nv, _ = counts.cpu().tolist()
        assert nv <= 0xffffffff
        out.append("iso %.2f: %d triangles, %d vertices (%.3f per triangle); list %.2f GB, indexed %.2f GB (%.2f GB with normals)" % (
            iso, nt, nv, nv / max(nt, 1), 36 * nt / 1e9, (12 * nt + 12 * nv) / 1e9, (12 * nt + 24 * nv) / 1e9))
        tri = torch.empty((max(nt, 1), 3, 3), dtype=torch.float32, device="cuda")
        vert = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
        norm = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
        idx = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
        kinds = {
            "list count": (lambda: soup(iso, None, 0), 0),
            "list full": (lambda: soup(iso, tri, nt), 36 * nt),
            "indexed count": (lambda: indexed(iso, False, None, None, 0, None, 0), 0),
            "indexed full": (lambda: indexed(iso, False, vert, None, nv, idx, nt), 12 * nv + 12 * nt),
            "indexed full + normals": (lambda: indexed(iso, False, vert, norm, nv, idx, nt), 24 * nv + 12 * nt),
            "indexed full + normals, map": (lambda: indexed(iso, True, vert, norm, nv, idx, nt), 24 * nv + 12 * nt),
            "indexed vertices": (lambda: indexed(iso, False, vert, None, nv, None, 0), 12 * nv),
            "indexed vertices + normals": (lambda: indexed(iso, False, vert, norm, nv, None, 0), 24 * nv),
            "indexed indices": (lambda: indexed(iso, False, None, None, 0, idx, nt), 12 * nt),
        }
        runs = alternate({k: fn for k, (fn, _) in kinds.items()}, calls, repeats)
        base = statistics.median(runs["list full"])
        for k, (_, nbytes) in kinds.items():
            m = statistics.median(runs[k])
            out.append("  %-28s %s ms  %6.3f GB written  %7.1f GB/s  (%5.2f x the list's full call)" % (k, fmt(runs[k]), nbytes / 1e9, nbytes / 1e9 / (m * 1e-3), m / base))
        torch.cuda.synchronize()
        assert counts.cpu().tolist() == [nt, nt, nv, 0] and list_counts.cpu().tolist() == [nt, nt]
        # the two calls describe one surface: a sample of triangles, de-indexed, against the list
        pick = torch.randint(0, max(nt, 1), (4096,), device="cuda")
        indexed(iso, False, vert, None, nv, idx, nt)
        assert nt == 0 or bool((vert[idx[pick].long() & 0xffffffff].view(torch.int32) == tri[pick].view(torch.int32)).all())
        del tri, vert, norm, idx
        torch.cuda.empty_cache()


def rocprof(args):
    rows = kernel_stats(__file__, ["--isos", args.isos, "--calls", "2", "--repeats", "1", "--out", os.devnull], 900)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_mesh_indexed.py --isos %s --calls 2 --repeats 1` on one MI355X, a run of its own:" % args.isos,
            "# the kernels of vkv_isosurface_mesh_indexed (k_meshi_*) and of vkv_isosurface_mesh (k_mesh_*) over all variants and isos, ms per dispatch"
            ] + stats_table(rows, ("k_mesh",))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--isos", default="0.2,0.5")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_mesh_indexed.py --isos %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (
            args.isos, args.calls, args.repeats)]
        measure(ctx, [float(t) for t in args.isos.split(",")], args.calls, args.repeats, lines)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="mesh_indexed_times.txt", rocprof_name="mesh_indexed_rocprof.txt")


if __name__ == "__main__":
    main()
