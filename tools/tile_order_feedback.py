"""Experiment (GPU): start order of the tiles of a vkv_render_batch launch from MEASURED tile costs.
A first launch (centre-of-image-first order) is traced; every frame's tiles are then re-ordered longest first by the largest wave
iteration count of the tile's four waves (what a renderer could feed back from the previous frame rendered into the same target),
handed to the library through the diagnostic hook vkv_debug_tile_orders, and the same launch is timed with both orders.

    python tools/tile_order_feedback.py [frames per launch] [launches in flight on as many streams]
"""
import sys, os, ctypes as C, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from vkvolume_amd import abi, lib, volume as V
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
nstreams = int(sys.argv[2]) if len(sys.argv) > 2 else 1
torch.cuda.set_device(0)
ctx = lib.Context(0)
v, tf, frame, skip = bench.build_scene(ctx, "c3")
fw, fh = frame
views = bench.cameras(v, fw / fh)
sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=skip, clip_distance=1.0, early_ray_termination=True), (fw, fh))
L = lib.load()
streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(nstreams - 1)]
sets = []
for s in range(nstreams):
    bufs = [torch.zeros((fh, fw, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    plist = []
    for j in range(n):
        q = sp.make_params(*views[j % 8])
        q.d_out_rgba8, q.d_out_color, q.d_out_counts, q.d_out_depth, q.d_in_depth, q.blend_over_target = bufs[j].data_ptr(), None, None, None, None, 0
        plist.append(q)
    sets.append((bufs, plist))
tiles = plist[0].tiles.tile_count
nblocks = ((tiles + 7) // 8) * 8 * n


def timed(reps=40):
    for _ in range(4):
        for s in range(nstreams):
            ctx.render_batch(sets[s][1], streams[s].cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        for s in range(nstreams):
            ctx.render_batch(sets[s][1], streams[s].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * nstreams * n) * 1e3


def traced():
    trace = torch.zeros((nblocks * 4, 10), dtype=torch.int64, device="cuda")
    L.vkv_debug_trace(ctx.handle, trace.data_ptr())
    ctx.render_batch(sets[0][1], streams[0].cuda_stream)
    torch.cuda.synchronize()
    L.vkv_debug_trace(ctx.handle, None)
    return trace.cpu().numpy()


base_ms = timed()
t = traced()
live = t[:, 1] > 0
print("centre-first order: %.4f ms per frame; traced launch span %.1f us" % (base_ms, (t[live, 1].max() - t[live, 0].min()) / 100.0))
# wave w of workgroup b: frame (b >> 3) % n, tile = low word of rec[3]
widx = np.nonzero(live)[0]
wg = widx // 4
f_of = (wg >> 3) % n
tile_of = (t[live, 3] & 0xffffffff).astype(np.int64)
cost = np.zeros((n, tiles), np.int64)
np.maximum.at(cost, (f_of, tile_of), t[live, 2].astype(np.int64))
orders = np.stack([np.argsort(-cost[f], kind="stable") for f in range(n)]).astype(np.uint32)
d_orders = torch.from_numpy(orders.astype(np.int64)).to(torch.int32).cuda().contiguous()  # bit pattern of uint32 below 2^31
ref = [b.clone() for b in sets[0][0]]
L.vkv_debug_tile_orders(ctx.handle, d_orders.data_ptr(), n, tiles)
fb_ms = timed()
t2 = traced()
live2 = t2[:, 1] > 0
print("longest-first order from the measured costs: %.4f ms per frame; traced launch span %.1f us" % (fb_ms, (t2[live2, 1].max() - t2[live2, 0].min()) / 100.0))
for a, b in zip(ref, sets[0][0]):
    assert torch.equal(a, b), "the start order changed a frame"
L.vkv_debug_tile_orders(ctx.handle, None, 0, 0)
print("frames identical; gain %.1f %%" % (100.0 * (base_ms / fb_ms - 1.0)))
