// jet-pbrt_amd/csrc/jp_projection_runtime.h -- camera projections (include/jetpbrt_amd.h "Projections", DESIGN.md "Projections"): the entry points.
// The definition itself -- JpProjectionPlan, the three rays -- is include/jp_projection.h, shared with the host; k_raygen_proj, k_raygen_list_proj, k_other, k_guides
// and k_camera_rays call it through projected_ray (jp_kernels.hip).  Included by jp_kernels.hip after the host runtime: the projection state of the context
// (jp_runtime.h) and proj_plan_of (jp_render.h) are all that the code before it reads.
#pragma once

namespace
{
int projection_check_status(const JpProjection* p)
{
	switch (jp_projection_check(p))
	{
	case 0: return JP_OK;
	case 1: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_projection: set JpProjection.struct_bytes to sizeof(JpProjection)");
	case 2: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_projection: kind must be JP_PROJ_PERSPECTIVE, _ORTHOGRAPHIC, _EQUIRECT or _FISHEYE (0 .. 3)");
	case 3: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_projection: ortho_scale must be finite and > 0 (0: the default, 1)");
	case 4: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_projection: fov_deg must be finite and in (0, 360] (0: the default, 180)");
	default: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_projection: fit must be JP_FIT_DIAGONAL, _WIDTH or _HEIGHT (0 .. 2)");
	}
}
}

extern "C" {

int jp_check_projection(const JpProjection* p)
{
	if (!p) return JP_OK;                                              // NULL: the pinhole
	return projection_check_status(p);
}

int jp_set_projection(JpContext* c, const JpProjection* p)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_projection: null context");
	if (p) if (const int e = projection_check_status(p); e != JP_OK) return e;
	c->proj = JpProjection(); c->proj_on = false;
	if (p && p->kind != JP_PROJ_PERSPECTIVE) { c->proj = *p; c->proj.struct_bytes = (int32_t)sizeof(JpProjection); c->proj_on = true; }   // read by the next jp_render* / jp_render_guides* / jp_camera_rays
	return JP_OK;
}

int jp_get_projection_info(JpContext* c, JpProjectionInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_projection_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_projection_info: set JpProjectionInfo.struct_bytes to sizeof(JpProjectionInfo)");
	JpProjectionInfo i; std::memset(&i, 0, sizeof(i));
	if (c->proj_on) { i.kind = c->proj.kind; i.ortho_scale = c->proj.ortho_scale; i.fov_deg = c->proj.fov_deg; i.fit = c->proj.fit; }
	i.projected_last_render = c->last_proj; i.gamma0_last_render = c->last_proj_gamma0;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_projection_plan(const JpCamera* cam, const JpProjection* p, void* plan_out, int64_t capacity, int64_t* bytes)
{
	if (!cam || !bytes) return fail(JP_ERR_INVALID_ARGUMENT, "jp_projection_plan: null argument");
	*bytes = 0;
	if (p) if (const int e = projection_check_status(p); e != JP_OK) return e;
	if (!p || p->kind == JP_PROJ_PERSPECTIVE) return JP_OK;
	JpProjectionPlan pp;
	if (const int e = proj_plan_status(cam, p, pp, "jp_projection_plan"); e != JP_OK) return e;
	*bytes = (int64_t)sizeof(pp);
	if (!plan_out) return JP_OK;
	if (capacity < (int64_t)sizeof(pp)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_projection_plan: capacity smaller than the plan");
	std::memcpy(plan_out, &pp, sizeof(pp));
	return JP_OK;
}

int jp_projection_rays(const JpCamera* cam, const JpProjection* p, int32_t n, const float* fxfy, float* origin, float* dir)
{
	if (!cam || n < 0 || !fxfy || !origin || !dir) return fail(JP_ERR_INVALID_ARGUMENT, "jp_projection_rays: null argument");
	if (p) if (const int e = projection_check_status(p); e != JP_OK) return e;
	const bool on = p && p->kind != JP_PROJ_PERSPECTIVE;
	JpProjectionPlan pp;
	if (on) if (const int e = proj_plan_status(cam, p, pp, "jp_projection_rays"); e != JP_OK) return e;
	for (int32_t i = 0; i < n; i++)
	{
		if (on) jp_projection_ray(cam, &pp, fxfy[2 * i], fxfy[2 * i + 1], origin + 3 * (size_t)i, dir + 3 * (size_t)i);
		else jp_pinhole_ray(cam, fxfy[2 * i], fxfy[2 * i + 1], origin + 3 * (size_t)i, dir + 3 * (size_t)i);
	}
	return JP_OK;
}

} // extern "C"
