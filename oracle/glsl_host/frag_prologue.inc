// Included by a generated fragment-shader source, inside the variant's namespace, BEFORE the shader text.  Own code, no shader text.
static bool     vkv_fragment_discarded; // set by `discard`
static bool     vkv_hook_reached;
static uint32_t vkv_counters[3];
static float    vkv_color_at_hook[4];
// prep.py inserts one call of this before the SHOW_NUM_SAMPLES epilogue: the text itself only outputs the scaled sum of its three local counters
// and overwrites out_color with it.  The hook hands the counters and the blended colour to the harness; it changes no value the shader computes.
#define VKV_FRAG_HOOK(n_volume, n_distance, n_empty)                                                     \
	do                                                                                                   \
	{                                                                                                    \
		vkv_hook_reached = true;                                                                         \
		vkv_counters[0] = (uint32_t) (n_volume), vkv_counters[1] = (uint32_t) (n_distance);              \
		vkv_counters[2] = (uint32_t) (n_empty);                                                          \
		vkv_color_at_hook[0] = out_color.x, vkv_color_at_hook[1] = out_color.y;                          \
		vkv_color_at_hook[2] = out_color.z, vkv_color_at_hook[3] = out_color.w;                          \
	} while (0)
// GLSL: a name is in scope only AFTER its initialiser, C++: from its declarator on.  prep.py routes the one use of a global that a local of the
// same name shadows inside its own initialiser through this.
#define VKV_GLOBAL(name) ::VKV_NS::name
