// Included by a generated fragment-shader source, inside the variant's namespace, after the shader text: binds the uniforms, samplers and
// interpolants (the globals that the text declares) and runs main() once per covered pixel.  Fragments share nothing: serial order is immaterial.
// Own code, no shader text.

static void vkv_load(mat4 &m, const float *src)
{
	for (int i = 0; i < 16; ++i)
		m.m[i] = src[i];
}

static void vkv_run(const VkvRefFragArgs *a)
{
	vkv_load(camera_uniform.view, a->view), vkv_load(camera_uniform.proj, a->proj), vkv_load(camera_uniform.view_proj_inv, a->view_proj_inv);
	vkv_load(camera_uniform.model, a->model), vkv_load(camera_uniform.model_inv, a->model_inv);
	ray_cast_uniform.cam_pos_tex = vec4(a->cam_pos_tex[0], a->cam_pos_tex[1], a->cam_pos_tex[2], a->cam_pos_tex[3]);
	ray_cast_uniform.block_size  = vec4(a->block_size[0], a->block_size[1], a->block_size[2], a->block_size[3]);
	transfer_function_uniform.sampling_factor         = a->tf.sampling_factor;
	transfer_function_uniform.voxel_alpha_factor      = a->tf.voxel_alpha_factor;
	transfer_function_uniform.grad_magnitude_modifier = a->tf.grad_magnitude_modifier;
	transfer_function_uniform.use_gradient            = a->tf.use_gradient != 0;
	volume            = sampler3D{a->volume, a->extent[0], a->extent[1], a->extent[2]};
	transfer_function = sampler2D{a->tf_rgba8, 256, 256};
#ifdef PRECOMPUTED_GRADIENT
	VKV_GLOBAL(gradient) = sampler3D{a->gradient, a->extent[0], a->extent[1], a->extent[2]};
#endif
#ifndef DISABLE_SKIP
#ifdef ANISOTROPIC_DISTANCE
	for (int k = 0; k < 8; ++k)
		distance_map[k] = usampler3D{a->maps[k], a->map_extent[0], a->map_extent[1], a->map_extent[2]};
#else
	distance_map[0] = usampler3D{a->maps[0], a->map_extent[0], a->map_extent[1], a->map_extent[2]};
#endif
#endif
	const size_t n = (size_t) a->width * (size_t) a->height;
	for (size_t p = 0; p < n; ++p)
	{
		float *   color  = a->out_color + 4 * p;
		uint32_t *counts = a->out_counts + 3 * p;
		color[0] = color[1] = color[2] = color[3] = 0.0f;
		counts[0] = counts[1] = counts[2] = 0u;
		a->out_depth[p]    = 0.0f;
		a->out_fragment[p] = 0;
		if (!(a->entry[4 * p + 3] > 0.0f))
			continue; // the rasteriser produces no fragment here
		ray_entry = vec3(a->entry[4 * p], a->entry[4 * p + 1], a->entry[4 * p + 2]);
		{ // the vertex shaders' position: proj * (view * (model * vec4(ray_entry - 0.5, 1))), always in the pinned matrix-vector form
			const int mode = g_pinned;
			g_pinned       = 1;
			position       = camera_uniform.proj * (camera_uniform.view * (camera_uniform.model * vec4(ray_entry - 0.5f, 1.0f)));
			g_pinned       = mode;
		}
#ifdef DEPTH_ATTACHMENT
		i_depth = subpassInput{a->in_depth[p]};
#endif
		vkv_fragment_discarded = false, vkv_hook_reached = false;
		out_color   = vec4(0.0f);
		gl_FragDepth = 0.0f;
		main();
		if (vkv_fragment_discarded)
			continue;
		a->out_fragment[p] = 1;
		a->out_depth[p]    = gl_FragDepth;
		if (vkv_hook_reached)
		{
			for (int c = 0; c < 4; ++c)
				color[c] = vkv_color_at_hook[c];
			for (int c = 0; c < 3; ++c)
				counts[c] = vkv_counters[c];
		}
		else
			color[0] = out_color.x, color[1] = out_color.y, color[2] = out_color.z, color[3] = out_color.w;
	}
}
static VkvRefRegisterFrag vkv_registered(VKV_VARIANT_KEY, vkv_run);
