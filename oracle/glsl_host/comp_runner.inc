// Included by a generated compute-shader source, inside the variant's namespace, after the shader text: binds the shader's resources (the
// globals that the text declares) and runs main() once per invocation of the dispatch, serially.  Own code, no shader text.
//
// Why serial execution is the same as the GPU's, per shader:
//   gradient_map.comp                reads `volume`, writes its own texel of `gradient_map`: two different images.
//   occupancy_map.comp               reads `volume` (+ `gradient_map`, the transfer function), writes its own cell of `occupancy_map`.
//   distance_map.comp                stage 0 runs with `dist` and `dist_swap` bound to the SAME image, but an invocation reads and writes only its
//                                    own row (fixed y, z), in program order; stage 1 reads `dist` and writes `dist_swap`, stage 2 the reverse.
//   distance_map_anisotropic.comp    stage 0 reads `dist_swap` and writes `dist`; when both are map 7 an invocation reads a texel of its own row
//                                    before it writes it; stages 1 and 2 read one image and write the other.
// No invocation ever reads what another invocation of the same dispatch writes, so no ordering between invocations matters.

static void vkv_run(const VkvRefCompArgs *a)
{
#if VKV_KIND == VKV_REF_COMP_GRADIENT
	volume       = image3D{a->image[0], a->extent[0], a->extent[1], a->extent[2]};
	gradient_map = image3D{a->image[1], a->extent[0], a->extent[1], a->extent[2]};
#elif VKV_KIND == VKV_REF_COMP_OCCUPANCY
	volume = image3D{a->image[0], a->extent[0], a->extent[1], a->extent[2]};
#ifdef PRECOMPUTED_GRADIENT
	gradient_map = image3D{a->image[1], a->extent[0], a->extent[1], a->extent[2]};
#endif
	occupancy_map = uimage3D{a->map, a->map_extent[0], a->map_extent[1], a->map_extent[2]};
	block_size    = ivec4(a->block[0], a->block[1], a->block[2], 0);
#else
	dist      = uimage3D{a->image[0], a->extent[0], a->extent[1], a->extent[2]};
	dist_swap = uimage3D{a->image[1], a->extent[0], a->extent[1], a->extent[2]};
	stage     = a->stage;
#if VKV_KIND == VKV_REF_COMP_DISTANCE_ANISO
	dir = a->dir;
#endif
#endif
#if VKV_KIND == VKV_REF_COMP_GRADIENT || VKV_KIND == VKV_REF_COMP_OCCUPANCY
	transfer_function = sampler2D{a->tf_rgba8, 256, 256};
	transfer_function_uniform.sampling_factor         = a->tf->sampling_factor;
	transfer_function_uniform.voxel_alpha_factor      = a->tf->voxel_alpha_factor;
	transfer_function_uniform.grad_magnitude_modifier = a->tf->grad_magnitude_modifier;
	transfer_function_uniform.use_gradient            = a->tf->use_gradient != 0;
#endif
	// the whole dispatch, the invocations past the image's edge included (each shader's first lines send them away)
	for (uint32_t z = 0; z < a->groups[2] * VKV_LOCAL_Z; ++z)
		for (uint32_t y = 0; y < a->groups[1] * 8u; ++y)
			for (uint32_t x = 0; x < a->groups[0] * 8u; ++x)
			{
				gl_GlobalInvocationID = uvec3(x, y, z);
				main();
			}
}
static VkvRefRegisterComp vkv_registered(VKV_KIND_SLOT, vkv_run);
