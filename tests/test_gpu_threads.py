"""GPU: the C ABI driven from several host threads at once (include/vkvolume_amd.h, "Conventions"; INTEGRATION.md, "One context, many
streams").  ctypes releases the GIL, so the entry points really run in parallel.  Every case computes its outputs serially first, in the
main thread, checks a subset of those against the CPU oracle, then runs the same work from threads that start together (one barrier), round
after round, and compares every output with the serial one, byte for byte.  Threads are daemons joined with a time limit; inside them only
return codes are checked (vkv_last_error is one buffer per context)."""
import random
import threading
import time

import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_gpu_parity import compare_render, make_gpu_volume
from tests.test_gpu_volume_region import SOURCES, make_source
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu

SHAPE = (96, 80, 72)          # w, h, d of every volume: one volume extent, one map extent, one tile schedule for all threads
SIZE = (256, 192)             # one frame size
BATCH = 4                     # frames per vkv_render_batch
JOIN_S = 120.0                # per thread and round: a thread still alive after this is a deadlock or a hang
PER_THREAD_STREAM = 2         # the handle of hipStreamPerThread
SKIPS = (abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE)


def _u8(*shape):
    return torch.empty(shape, dtype=torch.uint8, device="cuda")


class Worker:
    """One thread's share of the work: a volume of its own (seeded synthetic volume, gradient map, packed image), a transfer function of its
    own, and output buffers of its own - one set per skipping type, plus what the mixed sequence writes."""

    def __init__(self, ctx, k, skips, box_seed=0):
        self.k, self.skips = k, tuple(skips)
        opt = abi.VolumeOptions(intensity_min=0.08 + 0.015 * k, intensity_max=1.0, gradient_min=0.0, gradient_max=0.17 + 0.012 * k)
        self.opt, self.tfu = opt, lib.transfer_function_uniform(opt)
        self.scene = T.OracleScene(O.synth_volume(SHAPE, 1, 0x7E11 + 17 * k), opt, 4)
        self.v, _ = make_gpu_volume(ctx, self.scene)  # volume, gradient map, packed image, host-built texture + tables
        self.vol0, self.grad0, self.packed0 = self.v.volume.clone(), self.v.gradient.clone(), self.v.packed.clone()
        me = self.scene.map_extent
        self.mshape = (me.depth, me.height, me.width)
        w, h = SIZE
        self.out = {}
        for s in self.skips:
            self.out[s] = dict(tex=_u8(256, 256, 4), tables=torch.empty(abi.TF_BITS_WORDS, dtype=torch.int32, device="cuda"),
                               maps=[_u8(*self.mshape) for _ in range(8)], count=torch.empty(1, dtype=torch.int64, device="cuda"),
                               color=torch.empty((h, w, 4), dtype=torch.float32, device="cuda"), counts=torch.empty((h, w, 3), dtype=torch.int32, device="cuda"),
                               depth=torch.empty((h, w), dtype=torch.float32, device="cuda"), batch=[_u8(h, w, 4) for _ in range(BATCH)])
        self.swap, self.swap2 = _u8(*self.mshape), _u8(*self.mshape)
        # what only the mixed sequence writes (its skipping type: skips[0])
        self.mix = dict(grad=self.v.gradient, maps_cd=[_u8(*self.mshape) for _ in range(8)], hist=torch.empty((256, 256), dtype=torch.int64, device="cuda"),
                        summary=_u8(me.width * me.height * me.depth, abi.CELL_SUMMARY_BYTES), tex2=_u8(256, 256, 4),
                        tables2=torch.empty(abi.TF_BITS_WORDS, dtype=torch.int32, device="cuda"), maps2=[_u8(*self.mshape) for _ in range(8)],
                        count2=torch.empty(1, dtype=torch.int64, device="cuda"), unresolved=torch.empty(1, dtype=torch.int64, device="cuda"),
                        volume=self.v.volume, packed=self.v.packed, hist_after=torch.empty((256, 256), dtype=torch.int64, device="cuda"),
                        batch_after=[_u8(h, w, 4) for _ in range(BATCH)])
        rng = np.random.default_rng(4100 + box_seed)
        self.box = abi.Box(9 + 3 * k, 11, 13, 31, 21, 17)        # one box size for every thread
        self.source = SOURCES[k % len(SOURCES)]
        self.src = make_source(rng, self.source, self.box, empty_share=0.4)
        self.params = {s: self._params(s) for s in self.skips}
        self.params_after = self._batch_params(self.skips[0], self.mix["batch_after"])

    # -- render parameter blocks: this worker's volume, texture, tables and maps of skipping type s, its own targets --
    def _param(self, s, azimuth):
        ro = abi.RenderOptions(skipping_type=s, clip_distance=1.0)
        view, proj = T.orbit(azimuth, elevation=15.0 + 4.0 * self.k, image_size=SIZE)
        p = self.scene.params(view, proj, SIZE, ro)
        o = self.out[s]
        p.d_volume, p.d_gradient, p.d_packed_volume = self.v.volume.data_ptr(), self.v.gradient.data_ptr(), self.v.packed.data_ptr()
        p.d_transfer_function, p.d_transfer_function_bits = o["tex"].data_ptr(), o["tables"].data_ptr()
        for i in range(8):
            p.d_distance_maps[i] = o["maps"][i].data_ptr()
        return p

    def _batch_params(self, s, targets):
        plist = []
        for j, t in enumerate(targets):
            p = self._param(s, 37.0 * self.k + 71.0 * j + 5.0)
            p.d_out_rgba8 = t.data_ptr()
            plist.append(p)
        return plist

    def _params(self, s):
        o = self.out[s]
        single = self._param(s, 23.0 * self.k + 200.0)
        single.d_out_color, single.d_out_counts, single.d_out_depth = o["color"].data_ptr(), o["counts"].data_ptr(), o["depth"].data_ptr()
        return dict(single=single, batch=self._batch_params(s, o["batch"]))

    # -- the work: enqueue only (no torch call, no wait); `ctx` and the stream handle `h` are the caller's --
    def update_tf(self, ctx, h, s):
        o = self.out[s]
        ctx.update_transfer_function(self.opt, self.v.volume.data_ptr(), self.v.gradient.data_ptr(), self.scene.extent, o["tex"].data_ptr(),
                                     o["tables"].data_ptr(), [m.data_ptr() for m in o["maps"]], self.swap.data_ptr(), self.scene.map_extent, s,
                                     o["count"].data_ptr(), h)

    def light(self, ctx, h, single=True):
        """vkv_update_transfer_function, vkv_render and vkv_render_batch with every skipping type of the worker"""
        for s in self.skips:
            self.update_tf(ctx, h, s)
            if single:
                ctx.render(self.params[s]["single"], h)
            ctx.render_batch(self.params[s]["batch"], h)

    def mixed(self, ctx, h):
        """gradient + distance maps, both transfer-function updates, histogram, cell summary, both render entry points, a box of new voxels,
        the histogram and a batch of the changed volume"""
        s, m, o = self.skips[0], self.mix, self.out[self.skips[0]]
        vol, grad, e, me = self.v.volume.data_ptr(), self.v.gradient.data_ptr(), self.scene.extent, self.scene.map_extent
        ctx.gradient_map(vol, grad, e, self.tfu, h)
        ctx.compute_distance_map(vol, grad, self.v.transfer_function.data_ptr(), self.tfu, e, [t.data_ptr() for t in m["maps_cd"]],
                                 self.swap.data_ptr(), me, s, h)
        self.update_tf(ctx, h, s)
        ctx.volume_histogram(vol, grad, e, None, abi.HISTOGRAM_SET, m["hist"].data_ptr(), h)
        ctx.cell_summary(vol, grad, e, me, None, m["summary"].data_ptr(), h)
        ctx.update_transfer_function_from_summary(self.opt, vol, grad, e, m["tex2"].data_ptr(), m["tables2"].data_ptr(), [t.data_ptr() for t in m["maps2"]],
                                                  self.swap2.data_ptr(), me, s, m["count2"].data_ptr(), m["summary"].data_ptr(), m["hist"].data_ptr(),
                                                  m["unresolved"].data_ptr(), h)
        ctx.render(self.params[s]["single"], h)
        ctx.render_batch(self.params[s]["batch"], h)
        vt, big, (lo, hi) = self.source
        n = 8 if s == abi.SKIP_ANISOTROPIC_DISTANCE else 1
        ctx.update_volume_region(self.src.data_ptr(), vt, big, lo, hi, self.box, vol, grad, self.v.packed.data_ptr(), e, o["tex"].data_ptr(), self.tfu,
                                 [t.data_ptr() for t in o["maps"][:n]], self.swap.data_ptr(), me, s, h)
        ctx.volume_histogram(vol, grad, e, None, abi.HISTOGRAM_SET, m["hist_after"].data_ptr(), h)
        ctx.render_batch(self.params_after, h)

    # -- state between rounds (main thread) --
    def outputs(self):
        res = []
        for s in self.skips:
            for name, t in self.out[s].items():
                for i, x in enumerate(t if isinstance(t, list) else [t]):
                    res.append(("skip%d.%s%d" % (s, name, i), x))
        for name, t in self.mix.items():
            for i, x in enumerate(t if isinstance(t, list) else [t]):
                res.append(("mixed.%s%d" % (name, i), x))
        return res

    def reset(self):
        """sentinels in every output (a launch that writes another thread's targets leaves them behind), the volume as it was loaded"""
        for _, t in self.outputs():
            if t.dtype == torch.float32:
                t.fill_(-3.0)
            elif t.dtype == torch.uint8:
                t.fill_(0xA5)
            else:
                t.fill_(-77)
        self.v.volume.copy_(self.vol0)
        self.v.gradient.copy_(self.grad0)
        self.v.packed.copy_(self.packed0)

    def snapshot(self):
        return {name: t.clone() for name, t in self.outputs()}

    # -- the serial results against the oracle --
    def check_oracle(self, snap, mixed, single=True):
        sc = self.scene
        for s in self.skips:
            assert np.array_equal(snap["skip%d.tex0" % s].cpu().numpy(), sc.tex), "worker %d: texture" % self.k
            if not mixed:        # (the mixed sequence's box of new voxels rewrites these maps: its maps_cd / maps2 are checked below)
                for i, em in enumerate(sc.maps(s)):
                    assert np.array_equal(snap["skip%d.maps%d" % (s, i)].cpu().numpy(), em), "worker %d skip %d: map %d" % (self.k, s, i)
            assert int(snap["skip%d.count0" % s].item()) == O.occupied_voxel_count(sc.vol, sc.grad, sc.tf), "worker %d: count" % self.k
            if mixed and s != self.skips[0]:
                continue
            if single:
                got = (snap["skip%d.color0" % s].cpu().numpy(), snap["skip%d.counts0" % s].cpu().numpy().astype(np.uint32),
                       snap["skip%d.depth0" % s].cpu().numpy(), None)
                compare_render(got, sc.render(self.params[s]["single"]), "worker %d skip %d: vkv_render" % (self.k, s))
            ref = sc.render(self.params[s]["batch"][1], want_rgba8=True)
            assert np.array_equal(snap["skip%d.batch1" % s].cpu().numpy(), ref.rgba8), "worker %d skip %d: vkv_render_batch frame 1" % (self.k, s)
        if mixed:
            s = self.skips[0]
            for i, em in enumerate(sc.maps(s)):
                assert np.array_equal(snap["mixed.maps_cd%d" % i].cpu().numpy(), em), "worker %d: compute_distance_map %d" % (self.k, i)
                assert np.array_equal(snap["mixed.maps2%d" % i].cpu().numpy(), em), "worker %d: maps from the summary %d" % (self.k, i)
            assert np.array_equal(snap["mixed.tex20"].cpu().numpy(), sc.tex)
            assert torch.equal(snap["mixed.count20"], snap["skip%d.count0" % s]), "worker %d: count from the histogram" % self.k
            hist = np.bincount(sc.grad.astype(np.int64).ravel() * 256 + sc.vol.astype(np.int64).ravel(), minlength=65536).reshape(256, 256)
            assert np.array_equal(snap["mixed.hist0"].cpu().numpy(), hist), "worker %d: histogram" % self.k


def compare(workers, serial, label):
    """mismatching elements per output of every worker against its serial snapshot: {name: count}"""
    bad = {}
    for w, ref in zip(workers, serial):
        for name, t in w.outputs():
            n = int((t != ref[name]).sum().item())
            if n:
                bad["w%d.%s" % (w.k, name)] = bad.get("w%d.%s" % (w.k, name), 0) + n
    return bad


def run_rounds(fns, rounds, workers, serial, label, prepare=None):
    """`rounds` times: reset the workers, start one thread per fn on a barrier, join each with a time limit, compare every output."""
    mismatches = {}
    for r in range(rounds):
        for w in workers:
            w.reset()
        if prepare is not None:
            prepare(r)
        torch.cuda.synchronize()
        barrier = threading.Barrier(len(fns))
        errors = []

        def body(fn, r=r):
            try:
                barrier.wait(timeout=JOIN_S)
                fn(r)
            except BaseException as e:  # noqa: B902  (reported below, never swallowed)
                errors.append(repr(e))
                barrier.abort()

        threads = [threading.Thread(target=body, args=(fn,), daemon=True) for fn in fns]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_S)
        if any(t.is_alive() for t in threads):
            pytest.fail("%s, round %d: deadlock or hang (a thread is still alive after %g s)" % (label, r, JOIN_S))
        assert not errors, "%s, round %d: %s" % (label, r, errors[:4])
        torch.cuda.synchronize()
        for name, n in compare(workers, serial, label).items():
            mismatches[name] = mismatches.get(name, 0) + n
    assert not mismatches, "%s: outputs differ from the serial run (mismatching elements over %d rounds): %s" % (
        label, rounds, sorted(mismatches.items())[:40])


def serial_results(ctx, workers, work, check_first=2, mixed=False, single=True):
    """every worker's work once, alone, in the main thread; the first `check_first` against the oracle"""
    snaps = []
    for w in workers:
        w.reset()
        torch.cuda.synchronize()
        work(ctx, w)
        torch.cuda.synchronize()
        snaps.append(w.snapshot())
    for w, snap in list(zip(workers, snaps))[:check_first]:
        w.check_oracle(snap, mixed, single)
    return snaps


# ---------------------------------------------------------------------------------------------------------------------------------
# a. one context per thread, streams of its own (one host thread per GPU, each with its own context, rehearsed on one GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_threads", [2, 8])
def test_one_context_per_thread(ctx, n_threads):
    workers = [Worker(ctx, k, SKIPS) for k in range(n_threads)]
    serial = serial_results(ctx, workers, lambda c, w: w.light(c, torch.cuda.current_stream().cuda_stream))
    contexts = [lib.Context(0) for _ in range(n_threads)]
    streams = [torch.cuda.Stream() for _ in range(n_threads)]
    try:
        fns = [lambda r, w=w, c=c, s=s: w.light(c, s.cuda_stream) for w, c, s in zip(workers, contexts, streams)]
        run_rounds(fns, 4, workers, serial, "%d threads, a context each" % n_threads)
    finally:
        torch.cuda.synchronize()
        for c in contexts:
            c.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# b. / e. one context shared by 4 threads, a stream each; the first use of a frame size and a volume extent, vkv_prepare_render and
# vkv_register_target race the other threads' launches; (e) a fifth thread switches the tuning block all the while
# ---------------------------------------------------------------------------------------------------------------------------------
TUNING_SWITCHES = dict(address_tables=(0, 1, 2), wave_shape=(0, 4, 8, 16), clamp_always=(0, 1), scheduler=(0, 1), batch_mode=(0, 1), feedback=(0, 1))


@pytest.mark.parametrize("tuning_thread", [False, True], ids=["streams", "streams_and_tuning"])
def test_one_context_four_threads_own_streams(ctx, tuning_thread):
    workers = [Worker(ctx, k, (SKIPS[k % 4],), box_seed=k) for k in range(4)]
    serial = serial_results(ctx, workers, lambda c, w: w.mixed(c, torch.cuda.current_stream().cuda_stream), check_first=4, mixed=True)
    shared = lib.Context(0)        # has seen no frame size and no volume extent yet: the tables are made while the threads run
    streams = [torch.cuda.Stream() for _ in workers]
    stop, toggles = threading.Event(), [0]

    def tune():
        rng = random.Random(5)
        while not stop.is_set():
            shared.set_tuning(**{k: rng.choice(v) for k, v in TUNING_SWITCHES.items()})
            toggles[0] += 1
            time.sleep(0.0002)

    def work(r, w, s):
        if r == 0 and w.k < 2:        # set-up calls of two threads while the others launch
            st = w.skips[0]
            shared.prepare_render([w.params[st]["single"]] + w.params[st]["batch"], s.cuda_stream)
            shared.register_target(w.out[st]["color"].data_ptr(), SIZE, w.params[st]["single"].tiles)
        w.mixed(shared, s.cuda_stream)

    tuner = threading.Thread(target=tune, daemon=True) if tuning_thread else None
    try:
        if tuner is not None:
            tuner.start()
        run_rounds([lambda r, w=w, s=s: work(r, w, s) for w, s in zip(workers, streams)], 6, workers, serial,
                   "4 threads on one context" + (" with a tuning thread" if tuning_thread else ""))
    finally:
        stop.set()
        if tuner is not None:
            tuner.join(JOIN_S)
            assert not tuner.is_alive(), "tuning thread: deadlock or hang"
        torch.cuda.synchronize()
        shared.close()
    if tuning_thread:
        assert toggles[0] > 10, "the tuning thread hardly ran (%d switches)" % toggles[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# c. one context, 4 threads, ONE stream: the null stream (Volume's stream in a new thread) and one explicit torch stream.  Same volume
# extent, map extent, frame size, tile schedule, batch length and skipping type everywhere: an interleaving can only mix argument blocks of
# one shape into valid buffers (wrong bytes, never a stray pointer).
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["null_stream", "torch_stream"])
def test_one_context_four_threads_one_stream(ctx, which):
    workers = [Worker(ctx, k, (abi.SKIP_DISTANCE,), box_seed=10 + k) for k in range(4)]
    serial = serial_results(ctx, workers, lambda c, w: w.mixed(c, torch.cuda.current_stream().cuda_stream), check_first=1, mixed=True)
    s = torch.cuda.Stream() if which == "torch_stream" else None
    h = 0 if s is None else s.cuda_stream
    try:
        run_rounds([lambda r, w=w: w.mixed(ctx, h) for w in workers], 8, workers, serial, "4 threads on one %s" % which.replace("_", " "))
    finally:
        torch.cuda.synchronize()
        if s is not None:
            ctx.release_stream(h)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. hipStreamPerThread: one handle, a different stream in every thread
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_threads", [2, 4])
def test_per_thread_stream_handle(ctx, n_threads):
    workers = [Worker(ctx, k, SKIPS, box_seed=20 + k) for k in range(n_threads)]
    serial = serial_results(ctx, workers, lambda c, w: w.light(c, torch.cuda.current_stream().cuda_stream, single=False), check_first=1,
                            single=False)
    shared = lib.Context(0)

    def work(r, w):
        w.light(shared, PER_THREAD_STREAM, single=False)
        if r == 5:        # the last round: this thread's work done (the device-wide wait covers the per-thread streams), its block back
            torch.cuda.synchronize()
            shared.release_stream(PER_THREAD_STREAM)

    try:
        run_rounds([lambda r, w=w: work(r, w) for w in workers], 6, workers, serial, "%d threads on hipStreamPerThread" % n_threads)
    finally:
        torch.cuda.synchronize()
        shared.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# f. hipGraph capture in threads: two threads capture a vkv_render_batch each on their own stream and replay it while a third renders live
# ---------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_in_threads(ctx):
    st = abi.SKIP_DISTANCE
    workers = [Worker(ctx, k, (st,), box_seed=30 + k) for k in range(3)]
    serial = serial_results(ctx, workers, lambda c, w: w.light(c, torch.cuda.current_stream().cuda_stream), check_first=1)
    streams = [torch.cuda.Stream() for _ in workers]
    for w, s in zip(workers[:2], streams):
        ctx.prepare_render(w.params[st]["batch"], s.cuda_stream)
    torch.cuda.synchronize()
    reps = 5
    replays = [[[torch.empty_like(t) for t in w.out[st]["batch"]] for _ in range(reps)] for w in workers[:2]]
    capture_lock, errors, graphs = threading.Lock(), [], [None, None]

    def capture_and_replay(i):
        w, s = workers[i], streams[i]
        g = torch.cuda.CUDAGraph()
        with capture_lock:        # (torch.cuda.graph waits for the device on entry: not while another thread captures)
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                ctx.render_batch(w.params[st]["batch"], s.cuda_stream)
        with torch.cuda.stream(s):
            for rep in range(reps):
                for t in w.out[st]["batch"]:
                    t.fill_(0x5A)
                g.replay()
                for dst, src in zip(replays[i][rep], w.out[st]["batch"]):
                    dst.copy_(src)
        s.synchronize()
        graphs[i] = g

    def live(rounds=12):
        w, s = workers[2], streams[2]
        for _ in range(rounds):
            ctx.render_batch(w.params[st]["batch"], s.cuda_stream)
        s.synchronize()

    barrier = threading.Barrier(3)

    def body(fn):
        try:
            barrier.wait(timeout=JOIN_S)
            fn()
        except BaseException as e:  # noqa: B902
            errors.append(repr(e))
            barrier.abort()

    for w in workers:
        for t in w.out[st]["batch"]:
            t.fill_(0x5A)
    torch.cuda.synchronize()
    threads = [threading.Thread(target=body, args=(fn,), daemon=True) for fn in (lambda: capture_and_replay(0), lambda: capture_and_replay(1), live)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    if any(t.is_alive() for t in threads):
        pytest.fail("graph capture in threads: deadlock or hang")
    assert not errors, errors[:4]
    torch.cuda.synchronize()
    bad = []
    for i, w in enumerate(workers[:2]):
        for rep in range(reps):
            for j, t in enumerate(replays[i][rep]):
                n = int((t != serial[i]["skip%d.batch%d" % (st, j)]).sum().item())
                if n:
                    bad.append("worker %d replay %d frame %d: %d bytes" % (i, rep, j, n))
    for j, t in enumerate(workers[2].out[st]["batch"]):
        n = int((t != serial[2]["skip%d.batch%d" % (st, j)]).sum().item())
        if n:
            bad.append("live worker frame %d: %d bytes" % (j, n))
    del graphs[:]
    for s in streams:
        ctx.release_captured(s.cuda_stream)
        ctx.release_stream(s.cuda_stream)
    assert not bad, bad
