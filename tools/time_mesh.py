"""Cost of isosurface mesh extraction (vkv_isosurface_mesh: marching tetrahedra) on the bench's C3 volume.

C3 (1024x1024x795; bench.py's volume), per iso value:
  count dense / maxmap    the counting call (capacity 0: count + scan, no emit) without and with the max map (block 4), next to vkv_max_map and
                          vkv_gradient_map of the same volume in the same run: the project's other passes over one byte per voxel
  full dense / maxmap     the whole call with a capacity of the total (count + scan + emit), and the triangle count
GB/s counts the volume's bytes once (1 B read per voxel), for every row.
ms from device events (blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up
call of every variant; median [min .. max]).

    python tools/time_mesh.py [--isos 0.2,0.5] [--calls 10] [--repeats 7] [--out profiles/mesh_times.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, fmt, run, stream as st  # noqa: E402
from vkvolume_amd import lib  # noqa: E402


def measure(ctx, isos, calls, repeats, out):
    v, tf, _, _ = bench.build_scene(ctx, "c3")
    e, me = v.extent, v.map_extent
    n = e.width * e.height * e.depth
    vol, grad = v.volume, torch.empty_like(v.volume)
    max_map = v.build_max_map()
    scratch = torch.empty((lib.mesh_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    out.append("c3: volume %dx%dx%d (%.3f GB), max map %dx%dx%d, mesh scratch %.1f MB; ms per call, GB/s of the volume's bytes" % (
        e.width, e.height, e.depth, n / 1e9, me.width, me.height, me.depth, scratch.numel() * 8 / 1e6))

    def mesh(iso, skip, tri, capacity):
        ctx.isosurface_mesh(vol.data_ptr(), e, None, iso, max_map.data_ptr() if skip else None, me if skip else None, scratch.data_ptr(),
                            None if tri is None else tri.data_ptr(), capacity, counts.data_ptr(), st())

    for iso in isos:
        mesh(iso, False, None, 0)
        total = int(counts[0].item())
        below = 100.0 * float((max_map.float() * (1.0 / 255.0) < iso).float().mean().item())
        out.append("iso %.2f: %d triangles (%.2f GB of floats), %.1f %% of the max-map cells below iso" % (iso, total, 36 * total / 1e9, below))
        tri = torch.empty((max(total, 1), 3, 3), dtype=torch.float32, device="cuda")
        kinds = {
            "vkv_max_map": lambda: ctx.max_map(vol.data_ptr(), e, me, None, max_map.data_ptr(), st()),
            "vkv_gradient_map": lambda: ctx.gradient_map(vol.data_ptr(), grad.data_ptr(), e, tf, st()),
            "count dense": lambda: mesh(iso, False, None, 0),
            "count maxmap": lambda: mesh(iso, True, None, 0),
            "full dense": lambda: mesh(iso, False, tri, total),
            "full maxmap": lambda: mesh(iso, True, tri, total),
        }
        runs = alternate(kinds, calls, repeats)
        mm, gm = statistics.median(runs["vkv_max_map"]), statistics.median(runs["vkv_gradient_map"])
        for k in kinds:
            m = statistics.median(runs[k])
            out.append("  %-18s %s ms  %7.1f GB/s  (%5.2f x the max map, %5.2f x the gradient map)" % (k, fmt(runs[k]), n / 1e9 / (m * 1e-3), m / mm, m / gm))
        torch.cuda.synchronize()
        assert int(counts[0].item()) == total and int(counts[1].item()) == total
        del tri
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--isos", default="0.2,0.5")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_times.txt"))
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_mesh.py --isos %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (args.isos, args.calls, args.repeats)]
        measure(ctx, [float(t) for t in args.isos.split(",")], args.calls, args.repeats, lines)
        return lines

    run(args, plain)


if __name__ == "__main__":
    main()
