"""CPU: the ctypes binding (vkvolume_amd/lib.py) against its three yardsticks: the public headers, the public surface it had before its
entry points were gathered into one table, and the argument conversions that its wrappers still make.  No device is touched: the built
library is needed for lib.load() alone."""
import ctypes as C
import inspect
import json
import os
import re

import pytest

from vkvolume_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", n) for n in ("vkvolume_amd.h", "vkvolume_amd_debug.h")]
SURFACE = os.path.join(ROOT, "tests", "golden", "binding_surface.json")


# ---- a. header conformance -------------------------------------------------------------------------------------------------------------

PROTOTYPE = re.compile(r"(?:^|[;{}])\s*((?:const\s+)?\w+[\s*]+)(vkv_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)
PARAMETER = re.compile(r"^(const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)?\s*(\[\d*\])?$")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float}
RESULTS = {"int": C.c_int, "size_t": C.c_size_t, "const char *": C.c_char_p, "void": None}


def prototypes():
    """[(symbol, result text, [parameter text])] of every vkv_* function the two public headers declare, comments stripped"""
    found = []
    for header in HEADERS:
        src = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
        src = re.sub(r"//[^\n]*", " ", src)
        src = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", src, flags=re.M)  # preprocessor lines, continued ones included
        for result, symbol, params in PROTOTYPE.findall(src):
            params = [" ".join(p.split()) for p in params.split(",")]
            found.append((symbol, " ".join(result.replace("*", " * ").split()), [] if params == ["void"] else params))
    return found


def scalar_kind(t):
    """(bytes, 'float' / 'signed' / 'unsigned') of a ctypes scalar type; None for anything else"""
    code = getattr(t, "_type_", None)
    if not isinstance(code, str) or code not in "fdbhilqBHILQ":
        return None
    return C.sizeof(t), "float" if code in "fd" else "signed" if code.islower() else "unsigned"


def is_pointer_type(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def mismatches(symbol, result, params, restype, argtypes):
    """what is wrong with (restype, argtypes) as the binding of the prototype `result symbol(params)`: a list of messages, each naming the
    function and the parameter; empty when the binding conforms"""
    bad = []
    if result not in RESULTS:
        bad.append("%s: result type %r is none the binding knows" % (symbol, result))
    elif restype is not RESULTS[result]:
        bad.append("%s: returns %r but restype is %r" % (symbol, result, restype))
    argtypes = list(argtypes or [])
    if len(argtypes) != len(params):
        bad.append("%s: %d parameters declared but %d argtypes" % (symbol, len(params), len(argtypes)))
        return bad
    for i, (text, got) in enumerate(zip(params, argtypes)):
        where = "%s: parameter %d (`%s`) is bound as %r" % (symbol, i, text, got)
        m = PARAMETER.match(text)
        if m is None:
            bad.append("%s: parameter %d (`%s`) could not be parsed" % (symbol, i, text))
            continue
        const, base, stars, _, array = m.groups()
        mirror = getattr(abi, base[3:], None) if base.startswith("Vkv") else None
        if stars.strip() or array:  # a pointer or an array parameter
            if mirror is not None and stars.count("*") == 1 and not array:
                ok = got is C.c_void_p or got is C.POINTER(mirror)
            else:
                ok = got is C.c_void_p or is_pointer_type(got) or (got is C.c_char_p and const and base == "char" and stars.strip() == "*")
        elif base.startswith("Vkv"):
            ok = mirror is not None and got is mirror
        elif base in SCALARS:
            ok = scalar_kind(got) is not None and scalar_kind(got) == scalar_kind(SCALARS[base])
        else:
            ok = False
        if not ok:
            bad.append(where)
    return bad


def test_every_prototype_of_the_headers_matches_the_loaded_function():
    L = lib.load()
    protos = prototypes()
    assert len(protos) == len(lib.EXPORTS) + len(lib.DEBUG_EXPORTS)
    assert sorted(p[0] for p in protos) == sorted(lib.EXPORTS + lib.DEBUG_EXPORTS)
    bad = []
    for symbol, result, params in protos:
        f = getattr(L, symbol)
        bad += mismatches(symbol, result, params, f.restype, f.argtypes)
    assert not bad, "\n".join(bad)
    # the comparison can fail: the vkv_filter_volume row with its box and kind swapped shifts two parameters, and both are named
    symbol, result, params = next(p for p in protos if p[0] == "vkv_filter_volume")
    swapped = list(L.vkv_filter_volume.argtypes)
    assert swapped[4] is C.POINTER(abi.Box) and swapped[5] is C.c_int32
    swapped[4], swapped[5] = swapped[5], swapped[4]
    bad = mismatches(symbol, result, params, L.vkv_filter_volume.restype, swapped)
    assert len(bad) == 2 and all(b.startswith("vkv_filter_volume: parameter") for b in bad)
    assert "`const VkvBox *box`" in bad[0] and "`int32_t kind`" in bad[1]
    assert len(mismatches(symbol, result, params, C.c_size_t, swapped[:-1])) == 2  # the result type and the count


# ---- b. the public surface -------------------------------------------------------------------------------------------------------------

def public_callables():
    """{name: function} of lib's public functions and Context's public methods"""
    found = {n: f for n, f in vars(lib).items() if inspect.isfunction(f) and f.__module__ == lib.__name__ and not n.startswith("_")}
    found.update({"Context." + n: f for n, f in vars(lib.Context).items() if inspect.isfunction(f) and not n.startswith("_")})
    return found


def test_the_public_surface_is_what_it_was():
    """tests/golden/binding_surface.json was written once, at commit 2da65eb (the last one whose lib.py spelled every entry point out by
    hand), by a few lines of Python that were not kept: for every entry of public_callables() as it was there, str(inspect.signature(f)) and,
    for the names that do not end in _rc, f.__doc__."""
    want = json.load(open(SURFACE))
    have = public_callables()
    assert len(want) > 80
    for name, entry in want.items():
        assert name in have, name
        assert str(inspect.signature(have[name])) == entry["signature"], name
        assert have[name].__name__ == name.split(".")[-1], name
        if "doc" in entry:
            assert have[name].__doc__ == entry["doc"], name
    new = sorted(set(have) - set(want))
    assert all(n.endswith("_rc") for n in new), new


# ---- c. the conversions that remain ----------------------------------------------------------------------------------------------------

HANDLE = 0x1234


class Recorder:
    """stands in for the loaded library: every vkv_* attribute is a function that records its normalised arguments and returns `status`"""

    def __init__(self, status=0):
        self.status, self.calls = status, {}

    def __getattr__(self, name):
        if not name.startswith("vkv_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.setdefault(name, []).append(tuple(normalise(a) for a in args))
            return b"recorded message" if name == "vkv_last_error" else self.status
        return call

    def last(self, name):
        return self.calls[name][-1]


def normalise(a):
    """a structure, or a byref of one, as its bytes; a ctypes array as a list; a c_void_p as its value"""
    if type(a).__name__ == "CArgObject":
        a = a._obj
    if isinstance(a, C.Structure):
        return bytes(a)
    if isinstance(a, C.Array):
        return [normalise(x) for x in a]
    if isinstance(a, C.c_void_p):
        return a.value
    return a


def context(status=0):
    ctx = lib.Context.__new__(lib.Context)
    ctx._lib, ctx.handle, ctx.device = Recorder(status), C.c_void_p(HANDLE), 0
    return ctx, ctx._lib


EXT, MAP_EXT, NO_EXT = bytes(abi.Extent3D(40, 50, 60)), bytes(abi.Extent3D(10, 13, 15)), bytes(abi.Extent3D(0, 0, 0))
BOX = abi.Box(1, 2, 3, 4, 5, 6)


def ext():
    return abi.Extent3D(40, 50, 60)


def map_ext():
    return abi.Extent3D(10, 13, 15)


@pytest.mark.parametrize("box, c_box", [(None, None), (BOX, bytes(BOX))])
def test_absent_map_extent_and_box_of_the_box_calls(box, c_box):
    ctx, rec = context()
    assert ctx.isosurface_mesh_rc(10, ext(), box, 0.5, None, None, 11, 12, 7, 13, 99) == 0
    assert rec.last("vkv_isosurface_mesh") == (HANDLE, 10, EXT, c_box, 0.5, None, NO_EXT, 11, 12, 7, 13, 99)
    ctx.isosurface_mesh_rc(10, ext(), box, 0.5, 20, map_ext(), 11, 12, 7, 13)
    assert rec.last("vkv_isosurface_mesh") == (HANDLE, 10, EXT, c_box, 0.5, 20, MAP_EXT, 11, 12, 7, 13, 0)
    ctx.isosurface_mesh_indexed_rc(10, ext(), box, 0.5, None, None, 11, 12, 14, 100, 15, 200, 13, 99)
    assert rec.last("vkv_isosurface_mesh_indexed") == (HANDLE, 10, EXT, c_box, 0.5, None, NO_EXT, 11, 12, 14, 100, 15, 200, 13, 99)
    ctx.label_components_rc(10, ext(), box, 0.5, abi.CONNECT_26, None, None, 11, 12, 14, 9, 13, 99)
    assert rec.last("vkv_label_components") == (HANDLE, 10, EXT, c_box, 0.5, abi.CONNECT_26, None, NO_EXT, 11, 12, 14, 9, 13, 99)


def test_distance_limit():
    ctx, rec = context()
    ctx.distance_transform_rc(10, ext(), None, 0.5, abi.DISTANCE_TO_OUTSIDE, None, 11, 12, 99)
    assert rec.last("vkv_distance_transform") == (HANDLE, 10, EXT, None, 0.5, abi.DISTANCE_TO_OUTSIDE, abi.DISTANCE_NONE, 11, 12, 99)
    assert abi.DISTANCE_NONE == 0xffffffff
    ctx.distance_transform_rc(10, ext(), BOX, 0.5, abi.DISTANCE_TO_INSIDE, 7, 11, 12, 99)
    assert rec.last("vkv_distance_transform") == (HANDLE, 10, EXT, bytes(BOX), 0.5, abi.DISTANCE_TO_INSIDE, 7, 11, 12, 99)


def test_update_volume_region_flags_and_absent_structures():
    ctx, rec = context()
    tf = abi.TransferFunctionUniform()
    for big_endian, c_big in ((True, 1), (False, 0)):
        ctx.update_volume_region_rc(10, 2, big_endian, 0.0, 255.0, None, 11, 12, 13, ext(), 14, None, None, 15, map_ext(), 1, 99)
        assert rec.last("vkv_update_volume_region") == (HANDLE, 10, 2, c_big, 0.0, 255.0, None, 11, 12, 13, EXT, 14, None, None, 15, MAP_EXT, 1, 99)
    ctx.update_volume_region_rc(10, 2, False, 0.0, 255.0, BOX, 11, 12, 13, ext(), 14, tf, [21, 22], 15, map_ext(), 1, 99)
    assert rec.last("vkv_update_volume_region") == (HANDLE, 10, 2, 0, 0.0, 255.0, bytes(BOX), 11, 12, 13, EXT, 14, bytes(tf), [21, 22] + [None] * 6,
                                                    15, MAP_EXT, 1, 99)


def test_map_arrays():
    ctx, rec = context()
    tf, options = abi.TransferFunctionUniform(), abi.VolumeOptions(intensity_min=0.25)
    assert ctx.compute_distance_map(10, 12, 14, tf, ext(), [21], 15, map_ext(), 1, 99) is None
    assert rec.last("vkv_compute_distance_map") == (HANDLE, 10, 12, 14, bytes(tf), EXT, [21] + [None] * 7, 15, MAP_EXT, 1, 99)
    ctx.update_transfer_function_rc(options, 10, 12, ext(), 14, 16, None, 15, map_ext(), 1, None, 99)
    assert rec.last("vkv_update_transfer_function") == (HANDLE, bytes(options), 10, 12, EXT, 14, 16, None, 15, MAP_EXT, 1, None, 99)


def test_size_tuples_are_unpacked():
    ctx, rec = context()
    rect = abi.TileRect(1, 2, 3, 4)
    ctx.assemble_frame(1, 2, 3, (640, 480), (16, 8), 4, 1, 16, 0, 77, 99)
    assert rec.last("vkv_assemble_frame") == (HANDLE, 1, 2, 3, 640, 480, 16, 8, None, 4, 1, 16, 0, 77, 99)
    ctx.assemble_frame(1, 2, 3, (640, 480), (16, 8), 4, 1, 16, 0, 77, 99, rect=rect)
    assert rec.last("vkv_assemble_frame") == (HANDLE, 1, 2, 3, 640, 480, 16, 8, bytes(rect), 4, 1, 16, 0, 77, 99)
    ctx.scatter_tiles(2, 3, (640, 480), (16, 8), 4, 30, 16, 99)
    assert rec.last("vkv_scatter_tiles") == (HANDLE, 2, 3, 640, 480, 16, 8, None, 4, 30, 16, 99)
    ctx.scatter_tiles(2, 3, (640, 480), (16, 8), 4, 30, 16, rect=rect)
    assert rec.last("vkv_scatter_tiles") == (HANDLE, 2, 3, 640, 480, 16, 8, bytes(rect), 4, 30, 16, 0)
    tiles = abi.full_frame_tiles(640, 480)
    ctx.register_target(3, (640, 480), tiles)
    assert rec.last("vkv_register_target") == (HANDLE, 3, 640, 480, bytes(tiles))


def test_per_frame_arrays():
    ctx, rec = context()
    rects = [abi.TileRect(0, 0, 3, 4), abi.TileRect(1, 2, 5, 6)]
    ctx.assemble_frames(1, 2, [31, 32], 2, (640, 480), (16, 8), 4, 1, 16, 0, 77, 99, rects=rects, roots=[0, 3])
    assert rec.last("vkv_assemble_frames") == (HANDLE, 1, 2, [31, 32], 2, 640, 480, 16, 8, [bytes(r) for r in rects], 4, 1, 16, 0, [0, 3], 77, 99)
    ctx.assemble_frames(1, 2, None, 2, (640, 480), (16, 8), 4, 1, 16, 0, 77, 99)
    assert rec.last("vkv_assemble_frames") == (HANDLE, 1, 2, None, 2, 640, 480, 16, 8, None, 4, 1, 16, 0, None, 77, 99)
    blocks = [abi.RenderParams(), abi.RenderParams()]
    blocks[0].image_width, blocks[1].image_width = 640, 320
    ctx.render_batch(blocks, 99)
    assert rec.last("vkv_render_batch") == (HANDLE, [bytes(b) for b in blocks], 2, 99)
    ctx.prepare_render(blocks, 99)
    assert rec.last("vkv_prepare_render") == (HANDLE, [bytes(b) for b in blocks], 2, 99)
    assert bytes(blocks[0]) != bytes(blocks[1])


def test_raising_forms():
    params = abi.RenderParams()
    ctx, rec = context(0)
    assert ctx.render(params, 99) is None and ctx.render_rc(params, stream=99) == 0 and ctx.filter_volume(1, 2, ext(), None, 0) is None
    assert rec.calls["vkv_render"] == [(HANDLE, bytes(params), 99)] * 2 and "vkv_last_error" not in rec.calls
    ctx, rec = context(abi.VKV_E_UNSUPPORTED)
    assert ctx.render_rc(params) == abi.VKV_E_UNSUPPORTED and ctx.filter_volume_rc(1, 2, ext(), BOX, 1, 99) == abi.VKV_E_UNSUPPORTED
    assert rec.last("vkv_filter_volume") == (HANDLE, 1, 2, EXT, bytes(BOX), 1, 99)
    for call in (lambda: ctx.render(params), lambda: ctx.filter_volume(1, 2, ext(), None, 0, stream=99), lambda: ctx.render_batch([params])):
        with pytest.raises(lib.VkvError, match="recorded message") as e:
            call()
        assert e.value.code == abi.VKV_E_UNSUPPORTED
    assert rec.last("vkv_last_error") == (HANDLE,)
