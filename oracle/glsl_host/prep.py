#!/usr/bin/env python3
"""Turns the reference's GLSL shaders into C++ sources that compile against glsl_shim.hpp - one source per #define variant, each in a
namespace of its own, written ONLY below the output directory (oracle/_ref/gen; never committed).

This file holds no shader text.  Every change to the text is a regular expression anchored on a few tokens, with the number of places it must
match in that shader; a different number fails the build (the reference changed: look at it again).  The changes:

  * `#include "x"` is replaced by the file (so that the rules below reach it); `#version`, `#extension`, `precision` lines are dropped;
  * `layout(...)` declarations become plain declarations: a uniform block becomes a struct with the same members and instance name, a
    push-constant block (it has no instance name) becomes its members, a resource or an `in` / `out` variable loses its qualifiers, the
    work-group size line is dropped;
and three that go beyond declarations (DESIGN.md section 2 names them):
  * distance_map_anisotropic.comp reads `.x` of a scalar int, which C++ has no spelling for: the swizzle is dropped (same value);
  * one VKV_FRAG_HOOK(...) line is inserted before the SHOW_NUM_SAMPLES epilogue of the fragment shader, handing its three local counters to
    the harness (frag_prologue.inc) - the text itself only outputs their scaled sum;
  * in the fragment shader's get_gradient a local is initialised from the global sampler of the same name; in GLSL the local is not yet in
    scope there, in C++ it is: that one use names the global explicitly, VKV_GLOBAL(...).
"""
import os
import re
import sys

M = re.M
DROP_VERSION = ("#version", r"^[ \t]*#version[^\n]*\n", "")
DROP_EXTENSION = ("#extension", r"^[ \t]*#extension[^\n]*\n", "")
DROP_PRECISION = ("precision", r"^[ \t]*precision[ \t]+\w+[ \t]+\w+[ \t]*;[^\n]*\n", "")
DROP_LOCAL_SIZE = ("work-group size", r"^[ \t]*layout[ \t]*\([^)]*\)[ \t]*in[ \t]*;", "")
PUSH_CONSTANTS = ("push-constant block", r"layout[ \t]*\([ \t]*push_constant[^)]*\)[ \t]*uniform[ \t]+\w+\s*\{([^}]*)\}[ \t]*;", r"\1")
UNIFORM_BLOCK = ("uniform block", r"layout[ \t]*\([^)]*\)[ \t]*uniform[ \t]+(\w+)\s*\{", r"struct \1 {")
RESOURCE = ("resource", r"layout[ \t]*\([^)]*\)[ \t]*uniform[ \t]+(?:(?:mediump|highp|lowp)[ \t]+)?(\w+)[ \t]+(\w+)", r"\1 \2")
IN_OUT = ("in / out variable", r"layout[ \t]*\([^)]*\)[ \t]*(?:in|out)[ \t]+(\w+)[ \t]+(\w+)", r"\1 \2")
SCALAR_SWIZZLE = ("scalar swizzle", r"\bstart\.x\b", "start")
SHADOWED_GLOBAL = ("global shadowed in its own initialiser", r"texture\(gradient,", "texture(VKV_GLOBAL(gradient),")
COUNTER_HOOK = ("counter hook", r"^([ \t]*)(uint[ \t]+n_steps_max\b)",
                r"\1VKV_FRAG_HOOK(num_volume_samples, num_distance_samples, num_empty_samples);\n\1\2")

# shader -> (number of #include lines, [(rule, matches)]) - the rules run in this order, on the text with its includes resolved
SHADERS = {
    "gradient_map.comp": (2, [(DROP_VERSION, 1), (DROP_EXTENSION, 1), (DROP_LOCAL_SIZE, 1), (UNIFORM_BLOCK, 1), (RESOURCE, 3)]),
    "occupancy_map.comp": (2, [(DROP_VERSION, 1), (DROP_EXTENSION, 1), (DROP_LOCAL_SIZE, 1), (PUSH_CONSTANTS, 1), (UNIFORM_BLOCK, 1), (RESOURCE, 4)]),
    "distance_map.comp": (0, [(DROP_VERSION, 1), (DROP_LOCAL_SIZE, 1), (PUSH_CONSTANTS, 1), (RESOURCE, 2)]),
    "distance_map_anisotropic.comp": (0, [(DROP_VERSION, 1), (DROP_LOCAL_SIZE, 1), (PUSH_CONSTANTS, 1), (RESOURCE, 2), (SCALAR_SWIZZLE, 1)]),
    "volume_render.frag": (1, [(DROP_VERSION, 1), (DROP_EXTENSION, 1), (DROP_PRECISION, 1), (UNIFORM_BLOCK, 3), (RESOURCE, 6), (IN_OUT, 5),
                               (SHADOWED_GLOBAL, 1), (COUNTER_HOOK, 1)]),
}

# compute variants: (source name, shader, registry slot macro, local size z, defines)
COMP_VARIANTS = [
    ("comp_gradient", "gradient_map.comp", "VKV_REF_COMP_GRADIENT", "VKV_REF_COMP_GRADIENT", 8, []),
    ("comp_occupancy_0", "occupancy_map.comp", "VKV_REF_COMP_OCCUPANCY", "VKV_REF_COMP_OCCUPANCY", 8, []),
    ("comp_occupancy_1", "occupancy_map.comp", "VKV_REF_COMP_OCCUPANCY", "(VKV_REF_COMP_OCCUPANCY + 1)", 8, ["PRECOMPUTED_GRADIENT"]),
    ("comp_distance", "distance_map.comp", "VKV_REF_COMP_DISTANCE", "VKV_REF_COMP_DISTANCE", 1, []),
    ("comp_distance_aniso", "distance_map_anisotropic.comp", "VKV_REF_COMP_DISTANCE_ANISO", "VKV_REF_COMP_DISTANCE_ANISO", 1, []),
]
SKIP_DEFINES = [["DISABLE_SKIP"], ["BLOCK_SKIP"], [], ["ANISOTROPIC_DISTANCE"]]  # VolumeRenderSubpass, src/volume_render_subpass.cpp:57-92
SHOW_DEFINES = [[], ["SHOW_RAY_ENTRY"], ["SHOW_RAY_EXIT"]]


def frag_key(skip, no_ert, precomputed, depth, show):
    """harness.hpp, VKV_REF_FRAG_COUNT"""
    return skip | (no_ert << 2) | (precomputed << 3) | (depth << 4) | (show << 5)


def resolve_includes(shader_dir, name, expected):
    text = open(os.path.join(shader_dir, name)).read()
    found = []

    def put(m):
        found.append(m.group(1))
        return open(os.path.join(shader_dir, m.group(1))).read() + "\n"

    text = re.sub(r'^[ \t]*#include[ \t]+"([^"]+)"[^\n]*\n', put, text, flags=M)
    if len(found) != expected:
        raise SystemExit("prep.py: %s: %d #include lines, expected %d" % (name, len(found), expected))
    return text


def prepare(shader_dir, name):
    n_includes, rules = SHADERS[name]
    text = resolve_includes(shader_dir, name, n_includes)
    for (what, pattern, replacement), expected in rules:
        text, n = re.subn(pattern, replacement, text, flags=M)
        if n != expected:
            raise SystemExit("prep.py: %s: rule '%s' matched %d times, expected %d - the shader is not the one this recipe was written for"
                             % (name, what, n, expected))
    left = re.search(r"\blayout\b|^[ \t]*#(version|extension|include)\b", text, flags=M)
    if left:
        raise SystemExit("prep.py: %s: '%s' is left after all rules" % (name, left.group(0)))
    return text


def emit(path, namespace, head, defines, text, prologue, runner):
    lines = ["// generated by oracle/glsl_host/prep.py - holds the reference's shader text: never commit", '#include "harness.hpp"',
             '#include "glsl_shim.hpp"', "#define VKV_NS %s" % namespace]
    lines += head + ["#define %s" % d for d in defines]
    lines += ["namespace %s {" % namespace, "using namespace glsl;"]
    if prologue:
        lines.append('#include "%s"' % prologue)
    lines += [text, '#include "%s"' % runner, "}"]
    new = "\n".join(lines) + "\n"
    if not os.path.exists(path) or open(path).read() != new:  # an unchanged source keeps its time stamp: make compiles it once
        with open(path, "w") as f:
            f.write(new)
    return os.path.basename(path)


def main(argv):
    if len(argv) != 3:
        raise SystemExit("usage: prep.py <reference directory> <output directory>")
    shader_dir, out = os.path.join(argv[1], "shaders"), argv[2]
    os.makedirs(out, exist_ok=True)
    written = []
    texts = {name: prepare(shader_dir, name) for name in SHADERS}
    for source, shader, kind, slot, local_z, defines in COMP_VARIANTS:
        head = ["#define VKV_KIND %s" % kind, "#define VKV_KIND_SLOT %s" % slot, "#define VKV_LOCAL_Z %du" % local_z]
        written += emit(os.path.join(out, source + ".cpp"), "vkv_ref_" + source, head, defines, texts[shader], None, "comp_runner.inc"),
    for skip in range(4):
        for no_ert in range(2):
            for precomputed in range(2):
                for depth in range(2):
                    for show in range(3):
                        key = frag_key(skip, no_ert, precomputed, depth, show)
                        defines = SKIP_DEFINES[skip] + (["DISABLE_EARLY_RAY_TERMINATION"] if no_ert else []) + \
                            (["PRECOMPUTED_GRADIENT"] if precomputed else []) + (["DEPTH_ATTACHMENT"] if depth else []) + \
                            SHOW_DEFINES[show] + ["SHOW_NUM_SAMPLES"]
                        written += emit(os.path.join(out, "frag_%02d.cpp" % key), "vkv_ref_frag_%02d" % key, ["#define VKV_VARIANT_KEY %d" % key],
                                        defines, texts["volume_render.frag"], "frag_prologue.inc", "frag_runner.inc"),
    for f in os.listdir(out):  # sources and objects of variants that no longer exist
        if f.endswith((".cpp", ".o")) and os.path.splitext(f)[0] + ".cpp" not in written:
            os.remove(os.path.join(out, f))


if __name__ == "__main__":
    main(sys.argv)
