// jet-pbrt_amd/host/integrator.cc -- FGpuPathIntegrator::Render: the replacement for the reference's
// FIntegrator::Render (integrator.cc:35-80).  Instead of cutting the film into 20-row FRenderTasks for a
// std::thread pool (integrator.cc:53-74, parallel.cc), it flattens the scene once and calls the HIP library
// through the C ABI of include/jetpbrt_amd.h.  The HIP library is bound with dlopen so this host library has no
// link-time GPU dependency; if it is missing Render() fails loudly -- there is no CPU fallback.
#include "jetpbrt.h"

#include <dlfcn.h>
#include <cstring>
#include <mutex>

namespace jetpbrt
{
namespace
{
struct HipApi
{
	void* lib = nullptr;
	const char* (*last_error)() = nullptr;
	int (*create_context)(int, JpContext**) = nullptr;
	int (*destroy_context)(JpContext*) = nullptr;
	int (*upload_scene)(JpContext*, const JpScene*) = nullptr;
	int (*render)(JpContext*, const JpRenderParams*, float*) = nullptr;
	int (*render_rgb8)(JpContext*, const JpRenderParams*, uint8_t*, float*) = nullptr;
	int (*bsdf)(JpContext*, const JpBsdfDesc*, int32_t, const float*, const float*, const float*, const float*, float*, float*, float*, float*, float*, int32_t*) = nullptr;
	int (*get_counters)(JpContext*, JpCounters*) = nullptr;
	int (*abi_version)() = nullptr;
	int (*set_options)(JpContext*, const JpOptions*) = nullptr;
	int (*upload_scene_textured)(JpContext*, const JpScene*, const JpTextures*) = nullptr;   // (looked up, needed by textured scenes only)
	int (*render_variance)(JpContext*, const JpRenderParams*, float*, float*) = nullptr;                                                              // (FFilm::RequestVariance)
	int (*render_denoised_variance)(JpContext*, const JpRenderParams*, int32_t, const JpDenoiseParams*, float*, uint8_t*, float*, float*, float*, float*) = nullptr;   // (... with guides, the variance-guided filter or 8-bit bytes)
	int (*render_adaptive)(JpContext*, const JpRenderParams*, const JpAdaptive*, float*, int32_t*, float*) = nullptr;                                  // (FFilm::SetAdaptive)
	int (*render_guides)(JpContext*, const JpRenderParams*, int32_t, float*, float*, float*) = nullptr;                                               // (... with guides)
	int (*denoise_variance)(JpContext*, const JpDenoiseParams*, const float*, const float*, const float*, const float*, const float*, float*, float*) = nullptr;   // (... and the variance-guided filter)
	int (*render_denoised)(JpContext*, const JpRenderParams*, int32_t, const JpDenoiseParams*, float*, uint8_t*, float*, float*, float*) = nullptr;   // (looked up, needed by FFilm::RequestGuides / RequestDenoise only)
	int (*set_light_sampling)(JpContext*, const JpLightSampling*) = nullptr;                 // (looked up, needed by FScene::SetLightSampling only)
	int (*set_environment_map)(JpContext*, const JpEnvMap*) = nullptr;                       // (looked up, needed by FScene::SetEnvironmentMap only)
	int (*set_vertex_normals)(JpContext*, const JpVertexNormals*) = nullptr;                 // (looked up, needed by scenes with smooth meshes only)
	int (*set_normal_maps)(JpContext*, const JpNormalMaps*) = nullptr;                       // (looked up, needed by scenes with FMaterial::normalMap only)
	int (*set_texture_sampling)(JpContext*, const JpTextureSampling*) = nullptr;             // (looked up, needed by scenes with a sampling record only)
	int (*set_texture_procedurals)(JpContext*, const JpTextureProcedurals*) = nullptr;       // (looked up, needed by scenes with an FProceduralTexture only)
	int (*set_texture_mipmaps)(JpContext*, const JpTextureMipmaps*) = nullptr;               // (looked up, needed by scenes with FImageTexture::SetMipmaps only)
	int (*set_estimator)(JpContext*, const JpEstimator*) = nullptr;                        // (looked up, needed by FScene::SetEstimator only)
	int (*set_lens)(JpContext*, const JpLens*) = nullptr;                                    // (looked up, needed by FCamera::SetLens only)
	int (*set_projection)(JpContext*, const JpProjection*) = nullptr;                        // (looked up, needed by FCamera::SetProjection only)
	int (*check_projection)(const JpProjection*) = nullptr;
	int (*focus_distance)(JpContext*, float, float, float*) = nullptr;                       // (looked up, needed by FCamera::FocusAt only)
	int (*set_film)(JpContext*, const JpFilm*) = nullptr;                                    // (looked up, needed by FFilm::SetHDR / SetSampleClamp / SetToneMap only)
	int (*set_tonemap)(JpContext*, const JpToneMap*) = nullptr;                              // (looked up, needed by FFilm::SetToneMap only)
	int (*get_tonemap_info)(JpContext*, JpToneMapInfo*) = nullptr;
	std::string error;
};

HipApi& Api()
{
	static HipApi api; static std::once_flag once;
	std::call_once(once, []() {
		// libjetpbrt_amd.so lives next to this library's directory: <pkg>/csrc/libjetpbrt_amd.so
		std::string dir;
		Dl_info info;
		if (dladdr((void*)&Api, &info) && info.dli_fname) { dir = info.dli_fname; size_t p = dir.find_last_of('/'); dir = p == std::string::npos ? "." : dir.substr(0, p); }
		const char* env = getenv("JETPBRT_AMD_LIB");
		std::string cands[3] = { env ? env : "", dir + "/../csrc/libjetpbrt_amd.so", "libjetpbrt_amd.so" };
		for (auto& c : cands) { if (c.empty()) continue; api.lib = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL); if (api.lib) break; api.error = dlerror(); }
		if (!api.lib) return;
		api.last_error = (const char* (*)())dlsym(api.lib, "jp_last_error");
		api.create_context = (int (*)(int, JpContext**))dlsym(api.lib, "jp_create_context");
		api.destroy_context = (int (*)(JpContext*))dlsym(api.lib, "jp_destroy_context");
		api.upload_scene = (int (*)(JpContext*, const JpScene*))dlsym(api.lib, "jp_upload_scene");
		api.render = (int (*)(JpContext*, const JpRenderParams*, float*))dlsym(api.lib, "jp_render");
		api.get_counters = (int (*)(JpContext*, JpCounters*))dlsym(api.lib, "jp_get_counters");
		api.render_rgb8 = (int (*)(JpContext*, const JpRenderParams*, uint8_t*, float*))dlsym(api.lib, "jp_render_rgb8");
		api.bsdf = (decltype(api.bsdf))dlsym(api.lib, "jp_bsdf");
		api.abi_version = (int (*)())dlsym(api.lib, "jp_abi_version");
		api.set_options = (int (*)(JpContext*, const JpOptions*))dlsym(api.lib, "jp_set_options");
		api.upload_scene_textured = (int (*)(JpContext*, const JpScene*, const JpTextures*))dlsym(api.lib, "jp_upload_scene_textured");
		api.render_denoised = (decltype(api.render_denoised))dlsym(api.lib, "jp_render_denoised");
		api.render_variance = (decltype(api.render_variance))dlsym(api.lib, "jp_render_variance");
		api.render_denoised_variance = (decltype(api.render_denoised_variance))dlsym(api.lib, "jp_render_denoised_variance");
		api.render_adaptive = (decltype(api.render_adaptive))dlsym(api.lib, "jp_render_adaptive");
		api.render_guides = (decltype(api.render_guides))dlsym(api.lib, "jp_render_guides");
		api.denoise_variance = (decltype(api.denoise_variance))dlsym(api.lib, "jp_denoise_variance");
		api.set_light_sampling = (decltype(api.set_light_sampling))dlsym(api.lib, "jp_set_light_sampling");
		api.set_environment_map = (decltype(api.set_environment_map))dlsym(api.lib, "jp_set_environment_map");
		api.set_estimator = (decltype(api.set_estimator))dlsym(api.lib, "jp_set_estimator");
		api.set_vertex_normals = (decltype(api.set_vertex_normals))dlsym(api.lib, "jp_set_vertex_normals");
		api.set_lens = (decltype(api.set_lens))dlsym(api.lib, "jp_set_lens");
		api.set_normal_maps = (decltype(api.set_normal_maps))dlsym(api.lib, "jp_set_normal_maps");
		api.set_texture_sampling = (decltype(api.set_texture_sampling))dlsym(api.lib, "jp_set_texture_sampling");
		api.set_texture_mipmaps = (decltype(api.set_texture_mipmaps))dlsym(api.lib, "jp_set_texture_mipmaps");
		api.set_texture_procedurals = (decltype(api.set_texture_procedurals))dlsym(api.lib, "jp_set_texture_procedurals");
		api.focus_distance = (decltype(api.focus_distance))dlsym(api.lib, "jp_focus_distance");
		api.set_projection = (decltype(api.set_projection))dlsym(api.lib, "jp_set_projection");
		api.check_projection = (decltype(api.check_projection))dlsym(api.lib, "jp_check_projection");
		api.set_film = (decltype(api.set_film))dlsym(api.lib, "jp_set_film");
		api.set_tonemap = (decltype(api.set_tonemap))dlsym(api.lib, "jp_set_tonemap");
		api.get_tonemap_info = (decltype(api.get_tonemap_info))dlsym(api.lib, "jp_get_tonemap_info");
		if (!api.last_error || !api.create_context || !api.destroy_context || !api.upload_scene || !api.render || !api.get_counters || !api.render_rgb8 || !api.bsdf || !api.abi_version || !api.set_options)
		{ api.error = "libjetpbrt_amd.so lacks a required jp_* symbol"; dlclose(api.lib); api.lib = nullptr; }
		else if (api.abi_version() != JP_ABI_VERSION)            // a stale build would be handed structs of another size (JpCounters, JpBuildInfo, JpOptions)
		{ api.error = "libjetpbrt_amd.so implements ABI " + std::to_string(api.abi_version()) + ", this host library was built for ABI " + std::to_string(JP_ABI_VERSION); dlclose(api.lib); api.lib = nullptr; }
	});
	return api;
}
}

// ---- reflection API: one shading event on the device (jp_bsdf), on a context of this process created on first use ----
namespace
{
struct BsdfOut { float f[3], pdf, sf[3], swi[3], spdf; int32_t flags; bool ok; };
BsdfOut DeviceBsdf(const JpBsdfDesc& d, const FVector3& n, const FVector3& wo, const FVector3& wi, const FVector2& u)
{
	static JpContext* bctx = nullptr; static std::mutex mu;
	// the context lives on the device this process renders on (JETPBRT_DEVICE, else LOCAL_RANK, else 0 -- under HIP_VISIBLE_DEVICES
	// that is the rank's own GPU) and is destroyed at exit
	BsdfOut o; std::memset(&o, 0, sizeof(o));
	HipApi& api = Api();
	if (!api.lib) { fprintf(stderr, "FBSDF: HIP library not available (%s)\n", api.error.c_str()); return o; }
	std::lock_guard<std::mutex> lock(mu);
	if (!bctx)
	{
		int dev = 0;
		if (const char* e = getenv("JETPBRT_DEVICE")) dev = atoi(e); else if (const char* r = getenv("LOCAL_RANK")) dev = atoi(r);
		if (api.create_context(dev, &bctx) != JP_OK && (dev == 0 || api.create_context(0, &bctx) != JP_OK)) { fprintf(stderr, "FBSDF: %s\n", api.last_error()); bctx = nullptr; return o; }
		atexit([]() { if (bctx) { Api().destroy_context(bctx); bctx = nullptr; } });
	}
	const float nn[3] = { n.x, n.y, n.z }, a[3] = { wo.x, wo.y, wo.z }, b[3] = { wi.x, wi.y, wi.z }, uu[2] = { u.x, u.y };
	if (api.bsdf(bctx, &d, 1, nn, a, b, uu, o.f, &o.pdf, o.sf, o.swi, &o.spdf, &o.flags) != JP_OK) { fprintf(stderr, "FBSDF: %s\n", api.last_error()); return o; }
	o.ok = true;
	return o;
}
}
FColor FBSDF::Evalf(const FVector3& wo, const FVector3& wi) const { BsdfOut o = DeviceBsdf(desc, normal, wo, wi, FVector2(0.5f, 0.5f)); return FColor(o.f[0], o.f[1], o.f[2]); }
Float FBSDF::Pdf(const FVector3& wo, const FVector3& wi) const { return DeviceBsdf(desc, normal, wo, wi, FVector2(0.5f, 0.5f)).pdf; }
FBSDFSample FBSDF::Sample(const FVector3& wo, const FVector2& random) const
{
	BsdfOut o = DeviceBsdf(desc, normal, wo, wo, random);
	FBSDFSample s; s.f = FColor(o.sf[0], o.sf[1], o.sf[2]); s.wi = FVector3(o.swi[0], o.swi[1], o.swi[2]); s.pdf = o.spdf; s.ebsdf = o.flags;
	return s;
}

bool FCamera::CheckProjection(std::string* message) const
{
	HipApi& api = Api();
	if (!api.lib || !api.check_projection) { if (message) *message = api.lib ? "libjetpbrt_amd.so lacks jp_check_projection" : "HIP library not available (" + api.error + ")"; return false; }
	JpProjection p; p.struct_bytes = (int32_t)sizeof(p); p.kind = projKind; p.ortho_scale = projOrthoScale; p.fov_deg = projFovDeg; p.fit = projFit;
	if (api.check_projection(&p) == JP_OK) return true;
	if (message) *message = api.last_error();
	return false;
}

FGpuPathIntegrator::FGpuPathIntegrator(int maxDepth, int deviceId) : maxDepth(maxDepth), deviceId(deviceId) { std::memset(&counters, 0, sizeof(counters)); }

FGpuPathIntegrator::~FGpuPathIntegrator()
{
	if (ctx && Api().lib) Api().destroy_context(ctx);
}

void FGpuPathIntegrator::Render(const FScene* scene, FSampler* sampler, FFilm* film, int /*numthreads*/) const
{
	fprintf(stderr, "start rendering ...\n");                             // integrator.cc:44
	HipApi& api = Api();
	if (!api.lib) { fprintf(stderr, "FGpuPathIntegrator::Render: HIP library not available (%s); nothing rendered\n", api.error.c_str()); lastStatus = JP_ERR_NO_DEVICE; return; }
	if (!scene || !sampler || !film) { fprintf(stderr, "FGpuPathIntegrator::Render: null argument\n"); lastStatus = JP_ERR_INVALID_ARGUMENT; return; }
	if (!ctx) { lastStatus = api.create_context(deviceId, &ctx); if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); ctx = nullptr; return; } }
	if (optionsDirty) { lastStatus = api.set_options(ctx, &options); if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; } optionsDirty = false; }
	const FEnvironmentMap* const emap = scene->environmentMap && scene->environmentMap->Valid() ? scene->environmentMap.get() : nullptr;
	if (scene->environmentMap && !emap) { fprintf(stderr, "FGpuPathIntegrator::Render: FScene::SetEnvironmentMap was given an empty map\n"); lastStatus = JP_ERR_INVALID_ARGUMENT; return; }
	const unsigned long long envId = emap ? emap->id : 0;
	const bool mis = scene->estimator == JP_ESTIMATOR_MIS && kind == JP_INTEGRATOR_PATH;   // FScene::SetEstimator: the path integrator's (the other two render as they always did)
	const int lightMode = (emap || mis) ? JP_LIGHTS_POWER_ONE : scene->lightSampling;   // a mapped scene: the map light is an entry of the light table; MIS: the light strategy's pdf comes from it
	if (ctxEstimator != (mis ? JP_ESTIMATOR_MIS : JP_ESTIMATOR_NEE))
	{   // render-time state of the context: sent when it changes; a scene that never asked for MIS makes no such call
		if (!api.set_estimator) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_estimator\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
		JpEstimator es; es.struct_bytes = (int32_t)sizeof(es); es.mode = mis ? JP_ESTIMATOR_MIS : JP_ESTIMATOR_NEE;
		lastStatus = api.set_estimator(ctx, &es);
		if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
		ctxEstimator = es.mode;
	}
	if (uploaded != scene || uploadedLights != lightMode || uploadedEnv != envId || uploadedEnvUp != scene->environmentUp || uploadedEnvImp != scene->environmentImportance)
	{
		if (ctxEnv != envId || (envId && (ctxEnvUp != scene->environmentUp || ctxEnvImp != scene->environmentImportance)))
		{   // FScene::SetEnvironmentMap: the map goes to the context before the upload it is to affect (and leaves it the same way); a scene that never set one makes no such call
			if (!api.set_environment_map) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_environment_map\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			JpEnvMap m; std::memset(&m, 0, sizeof(m));
			if (emap) { m.struct_bytes = (int32_t)sizeof(m); m.width = emap->width; m.height = emap->height; m.up_axis = scene->environmentUp; m.importance = scene->environmentImportance; m.rgb = emap->data.data(); }
			lastStatus = api.set_environment_map(ctx, emap ? &m : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxEnv = envId; ctxEnvUp = scene->environmentUp; ctxEnvImp = scene->environmentImportance; uploaded = nullptr;
		}
		if (ctxLights != lightMode)
		{   // FScene::SetLightSampling: the mode goes to the context before the upload it is to affect; a scene that never set one makes no such call
			if (!api.set_light_sampling) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_light_sampling\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			JpLightSampling ls; ls.struct_bytes = (int32_t)sizeof(ls); ls.mode = lightMode;
			lastStatus = api.set_light_sampling(ctx, &ls);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxLights = lightMode; uploaded = nullptr;
		}
		FlatScene flat; std::string err;
		if (!FlattenScene(*scene, flat, &err)) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", err.c_str()); lastStatus = JP_ERR_INVALID_ARGUMENT; return; }
		if (flat.n_smooth > 0 || ctxNormals)
		{   // FSmoothing: the vertex normals go to the context before the upload they are to affect (and leave it the same way); a scene of flat meshes makes no such call
			if (!api.set_vertex_normals) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_vertex_normals\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_vertex_normals(ctx, flat.n_smooth > 0 ? &flat.normals : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxNormals = flat.n_smooth > 0;
		}
		if (flat.n_normal_mapped > 0 || ctxNormalMaps)
		{   // FMaterial::normalMap: the maps go to the context before the upload they are to affect (and leave it the same way); a scene without one makes no such call
			if (!api.set_normal_maps) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_normal_maps\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_normal_maps(ctx, flat.n_normal_mapped > 0 ? &flat.normalMaps : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxNormalMaps = flat.n_normal_mapped > 0;
		}
		if (flat.n_sampled > 0 || ctxSampling)
		{   // FImageTexture / FNormalMap::SetSampling: the records go to the context before the upload they are to affect; a scene whose records are all the identity removes
			// what an earlier scene left (NULL), and a context that never held any makes no such call
			if (!api.set_texture_sampling) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_texture_sampling\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_texture_sampling(ctx, flat.n_sampled > 0 ? &flat.sampling : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxSampling = flat.n_sampled > 0;
		}
		if (flat.n_mipmapped > 0 || ctxMipmaps)
		{   // FImageTexture::SetMipmaps / FScene::SetTextureMipmapDefault: the modes go to the context before the upload they are to affect; a scene without them removes what an
			// earlier scene left (NULL), and a context that never held any makes no such call
			if (!api.set_texture_mipmaps) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_texture_mipmaps\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_texture_mipmaps(ctx, flat.n_mipmapped > 0 ? &flat.mipmaps : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxMipmaps = flat.n_mipmapped > 0;
		}
		if (flat.n_procedural > 0 || ctxProcedurals)
		{   // FProceduralTexture: the records go to the context before the upload they are to affect, like the mipmap modes
			if (!api.set_texture_procedurals) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_texture_procedurals\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_texture_procedurals(ctx, flat.n_procedural > 0 ? &flat.procedurals : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxProcedurals = flat.n_procedural > 0;
		}
		// a scene with a textured material goes through jp_upload_scene_textured; any other makes exactly the calls it always made
		const bool textured = flat.textures.n_textures > 0;
		if (textured && !api.upload_scene_textured) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_upload_scene_textured\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
		auto upload = [&]() { return textured ? api.upload_scene_textured(ctx, &flat.view, &flat.textures) : api.upload_scene(ctx, &flat.view); };
		lastStatus = upload();
		if (lastStatus == JP_ERR_UNSUPPORTED && flat.view.n_bvh_nodes == 0)
		{   // FScene::deviceBuild, but the device-built tree was refused (deeper than the traversal stack): build the SAH tree
			// on the host for this upload -- a different hierarchy, the same GPU path
			fprintf(stderr, "FGpuPathIntegrator::Render: %s; building the hierarchy on the host instead\n", api.last_error());
			std::vector<FBounds3> pb; pb.reserve(scene->primitives.size());
			for (auto& p : scene->primitives) pb.push_back(p->shape->tightBox);
			BuildBVH(pb, flat.bvh, 4);
			flat.view.n_bvh_nodes = (int)flat.bvh.left.size(); flat.view.bvh_bounds = flat.bvh.bounds.data(); flat.view.bvh_left = flat.bvh.left.data(); flat.view.bvh_right = flat.bvh.right.data();
			flat.view.n_bvh_prim_indices = (int)flat.bvh.prim_index.size(); flat.view.bvh_prim_index = flat.bvh.prim_index.data();
			lastStatus = upload();
		}
		if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); uploaded = nullptr; return; }
		uploaded = scene; uploadedLights = lightMode; uploadedEnv = envId; uploadedEnvUp = scene->environmentUp; uploadedEnvImp = scene->environmentImportance;
	}
	{   // FCamera::SetLens / FocusAt: render-time state of the context, sent when it changes; a camera that never asked for a lens makes no such call
		const FCamera* cam = scene->Camera();
		JpLens l; std::memset(&l, 0, sizeof(l));
		if (cam && cam->lensRadius != 0)
		{
			l.struct_bytes = (int32_t)sizeof(l); l.radius = cam->lensRadius; l.focus_distance = cam->lensFocus; l.blades = cam->lensBlades; l.rotation_deg = cam->lensRotation;
			if (cam->focusAt)
			{   // autofocus on the uploaded scene: the pinhole ray through the film position
				if (!api.focus_distance) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_focus_distance\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
				float f = 0.f;
				lastStatus = api.focus_distance(ctx, cam->focusFx, cam->focusFy, &f);
				if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
				if (!(f > 0.f)) { fprintf(stderr, "FGpuPathIntegrator::Render: FCamera::FocusAt(%g, %g): the ray through that film position hits nothing to focus on\n", cam->focusFx, cam->focusFy); lastStatus = JP_ERR_INVALID_ARGUMENT; return; }
				l.focus_distance = f;
			}
			cam->lastFocus = l.focus_distance;
		}
		if (std::memcmp(&l, &ctxLens, sizeof(l)) != 0)
		{
			if (!api.set_lens) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_lens\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_lens(ctx, l.struct_bytes ? &l : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxLens = l;
		}
	}
	{   // FCamera::SetProjection: render-time state of the context, sent when it changes; a camera that never asked for a projection makes no such call
		const FCamera* cam = scene->Camera();
		JpProjection p; std::memset(&p, 0, sizeof(p));
		if (cam && cam->projKind != JP_PROJ_PERSPECTIVE) { p.struct_bytes = (int32_t)sizeof(p); p.kind = cam->projKind; p.ortho_scale = cam->projOrthoScale; p.fov_deg = cam->projFovDeg; p.fit = cam->projFit; }
		if (std::memcmp(&p, &ctxProjection, sizeof(p)) != 0)
		{
			if (!api.set_projection) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_projection\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_projection(ctx, p.struct_bytes ? &p : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxProjection = p;
		}
	}
	{   // FFilm::SetHDR / SetSampleClamp / SetToneMap: render-time state of the context, sent when it changes; a film that never asked for either makes no such call
		JpFilm f; std::memset(&f, 0, sizeof(f));
		if (film->hdr || film->sampleClamp != 0) { f.struct_bytes = (int32_t)sizeof(f); f.hdr = film->hdr ? 1 : 0; f.sample_clamp = film->sampleClamp; }
		if (std::memcmp(&f, &ctxFilm, sizeof(f)) != 0)
		{
			if (!api.set_film) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_film\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_film(ctx, f.struct_bytes ? &f : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxFilm = f;
		}
		JpToneMap t; std::memset(&t, 0, sizeof(t));
		if (film->haveToneMap)
		{
			const FToneMap& m = film->toneMap;
			t.struct_bytes = (int32_t)sizeof(t); t.curve = m.curve; t.exposure_mode = m.autoExposure ? JP_EXPOSURE_AUTO : JP_EXPOSURE_MANUAL;
			t.ev = m.ev; t.key = m.key; t.white = m.white; t.pct_low = m.pctLow; t.pct_high = m.pctHigh;
		}
		if (std::memcmp(&t, &ctxToneMap, sizeof(t)) != 0)
		{
			if (!api.set_tonemap || !api.get_tonemap_info) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_set_tonemap\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
			lastStatus = api.set_tonemap(ctx, t.struct_bytes ? &t : nullptr);
			if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
			ctxToneMap = t;
		}
	}
	const bool wantLDR = film->wantLDR || film->haveToneMap;           // a tone map: the 8-bit bytes come from the device's display transform, next to the fp32 film
	JpRenderParams rp; std::memset(&rp, 0, sizeof(rp));
	rp.width = film->Width(); rp.height = film->Height();
	rp.spp = sampler->GetSamplesPerPixel(); rp.max_depth = maxDepth;
	rp.sampler_mode = sampler->Mode(); rp.seed = sampler->Seed();
	rp.band_rows = bandRows; rp.shard_index = shardIndex; rp.shard_count = shardCount; rp.integrator = kind;
	const bool floatFilm = !(film->wantLDR && film->ldrOnly);
	std::vector<float> rgb(floatFilm ? (size_t)rp.width * rp.height * 3 : 0);
	std::vector<uint8_t> ldr;
	std::vector<float> galb, gnrm, gdep, gvar;
	const bool varFilter = film->wantDenoise && film->denoise.varianceGuided, wantVar = film->wantVariance || varFilter;
	if (wantVar && film->wantDenoise && !varFilter)
	{ fprintf(stderr, "FGpuPathIntegrator::Render: RequestVariance with RequestDenoise needs the variance-guided filter (FDenoiseOptions::varianceGuided)\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
	std::vector<int32_t> gcnt; bool countersRead = false;
	if (film->wantAdaptive)
	{   // FFilm::SetAdaptive: the adaptive render delivers the film, the counts and its own variance plane; guides and the variance-guided filter follow as calls of their own
		if (!api.render_adaptive || !api.render_guides || !api.denoise_variance) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_render_adaptive\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
		if (film->wantDenoise && !varFilter) { fprintf(stderr, "FGpuPathIntegrator::Render: SetAdaptive with RequestDenoise needs the variance-guided filter (FDenoiseOptions::varianceGuided)\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
		if (wantLDR) { fprintf(stderr, "FGpuPathIntegrator::Render: SetAdaptive delivers the fp32 film (no device tone map / RequestDeviceLDR with it)\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
		const size_t n = (size_t)rp.width * rp.height;
		gvar.assign(n, 0.f); gcnt.assign(n, 0);
		JpAdaptive ad; std::memset(&ad, 0, sizeof(ad));
		ad.struct_bytes = (int32_t)sizeof(ad); ad.min_spp = film->adaptMin; ad.step_spp = film->adaptStep; ad.max_spp = 0; ad.threshold = film->adaptThreshold; ad.dilate = film->adaptDilate ? 1 : 0;
		lastStatus = api.render_adaptive(ctx, &rp, &ad, rgb.data(), gcnt.data(), gvar.data());
		if (lastStatus == JP_OK) { api.get_counters(ctx, &counters); countersRead = true; }   // (before the guides' render: the counters are the adaptive render's)
		if (lastStatus == JP_OK && film->wantGuides)
		{
			galb.assign(3 * n, 0.f); gnrm.assign(3 * n, 0.f); gdep.assign(n, 0.f);
			lastStatus = api.render_guides(ctx, &rp, film->guideSpp_, galb.data(), gnrm.data(), gdep.data());
			if (lastStatus == JP_OK && varFilter)
			{
				JpDenoiseParams dp; std::memset(&dp, 0, sizeof(dp));
				dp.struct_bytes = (int32_t)sizeof(dp); dp.width = rp.width; dp.height = rp.height; dp.iterations = film->denoise.iterations;
				dp.sigma_color = film->denoise.sigmaColor; dp.sigma_normal = film->denoise.sigmaNormal; dp.sigma_depth = film->denoise.sigmaDepth; dp.demodulate = film->denoise.demodulate ? 1 : -1;
				std::vector<float> out(3 * n);
				lastStatus = api.denoise_variance(ctx, &dp, rgb.data(), galb.data(), gnrm.data(), gdep.data(), gvar.data(), out.data(), nullptr);
				if (lastStatus == JP_OK) rgb.swap(out);
			}
		}
	}
	else if (wantVar && (film->wantGuides || wantLDR))
	{   // FFilm::RequestVariance / the variance-guided RequestDenoise: the variance render, guides, filter and tone map in one call (no guides asked for: one camera sample of them, dropped)
		if (!api.render_denoised_variance) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_render_denoised_variance\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
		const size_t n = (size_t)rp.width * rp.height;
		gvar.assign(n, 0.f);
		if (film->wantGuides) { galb.assign(3 * n, 0.f); gnrm.assign(3 * n, 0.f); gdep.assign(n, 0.f); }
		if (wantLDR) ldr.assign(3 * n, 0);
		JpDenoiseParams dp; std::memset(&dp, 0, sizeof(dp));
		dp.struct_bytes = (int32_t)sizeof(dp); dp.width = rp.width; dp.height = rp.height; dp.iterations = film->denoise.iterations;
		dp.sigma_color = film->denoise.sigmaColor; dp.sigma_normal = film->denoise.sigmaNormal; dp.sigma_depth = film->denoise.sigmaDepth; dp.demodulate = film->denoise.demodulate ? 1 : -1;
		lastStatus = api.render_denoised_variance(ctx, &rp, film->wantGuides ? film->guideSpp_ : 1, varFilter ? &dp : nullptr, floatFilm ? rgb.data() : nullptr, wantLDR ? ldr.data() : nullptr,
		                                          film->wantGuides ? galb.data() : nullptr, film->wantGuides ? gnrm.data() : nullptr, film->wantGuides ? gdep.data() : nullptr, gvar.data());
	}
	else if (wantVar)
	{
		if (!api.render_variance) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_render_variance\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
		gvar.assign((size_t)rp.width * rp.height, 0.f);
		lastStatus = api.render_variance(ctx, &rp, rgb.data(), gvar.data());
	}
	else if (film->wantGuides)
	{   // FFilm::RequestGuides / RequestDenoise: render, guides, filter and tone map in one call -- the film stays on the device in between
		if (!api.render_denoised) { fprintf(stderr, "FGpuPathIntegrator::Render: libjetpbrt_amd.so lacks jp_render_denoised\n"); lastStatus = JP_ERR_UNSUPPORTED; return; }
		const size_t n = (size_t)rp.width * rp.height;
		galb.assign(3 * n, 0.f); gnrm.assign(3 * n, 0.f); gdep.assign(n, 0.f);
		if (wantLDR) ldr.assign(3 * n, 0);
		JpDenoiseParams dp; std::memset(&dp, 0, sizeof(dp));
		dp.struct_bytes = (int32_t)sizeof(dp); dp.width = rp.width; dp.height = rp.height; dp.iterations = film->denoise.iterations;
		dp.sigma_color = film->denoise.sigmaColor; dp.sigma_normal = film->denoise.sigmaNormal; dp.sigma_depth = film->denoise.sigmaDepth; dp.demodulate = film->denoise.demodulate ? 1 : -1;
		lastStatus = api.render_denoised(ctx, &rp, film->guideSpp_, film->wantDenoise ? &dp : nullptr, floatFilm ? rgb.data() : nullptr, wantLDR ? ldr.data() : nullptr, galb.data(), gnrm.data(), gdep.data());
	}
	else if (wantLDR)
	{   // FFilm::RequestDeviceLDR: gamma_encoding (film.h:24) runs on the GPU, the film comes back as 3 bytes per pixel
		ldr.assign((size_t)rp.width * rp.height * 3, 0);
		lastStatus = api.render_rgb8(ctx, &rp, ldr.data(), floatFilm ? rgb.data() : nullptr);
	}
	else lastStatus = api.render(ctx, &rp, rgb.data());
	if (lastStatus != JP_OK) { fprintf(stderr, "FGpuPathIntegrator::Render: %s\n", api.last_error()); return; }
	if (floatFilm)
		for (int y = 0; y < rp.height; y++) for (int x = 0; x < rp.width; x++)
		{
			const float* p = &rgb[3 * ((size_t)y * rp.width + x)];
			film->AddColor(x, y, FColor(p[0], p[1], p[2]));               // integrator.cc:108 / film.h:64-68
		}
	if (film->wantGuides)
	{
		const size_t n = (size_t)rp.width * rp.height;
		film->albedo.resize(n); film->normal.resize(n); film->depth.swap(gdep);
		for (size_t i = 0; i < n; i++) { film->albedo[i] = FColor(galb[3 * i], galb[3 * i + 1], galb[3 * i + 2]); film->normal[i] = FVector3(gnrm[3 * i], gnrm[3 * i + 1], gnrm[3 * i + 2]); }
	}
	if (wantVar || film->wantAdaptive) film->variance.swap(gvar);
	if (film->wantAdaptive) film->sampleCounts.swap(gcnt);
	if (wantLDR) { film->ldr8.swap(ldr); film->floatValid = floatFilm; }   // (after AddColor: any later change of a pixel drops the bytes again)
	if (film->haveToneMap)
	{   // FFilm::ToneMapScale: the exposure scale the transform used
		JpToneMapInfo ti; std::memset(&ti, 0, sizeof(ti)); ti.struct_bytes = (int32_t)sizeof(ti);
		if (api.get_tonemap_info(ctx, &ti) == JP_OK) film->toneMapScale = ti.scale_last;
	}
	if (!countersRead) api.get_counters(ctx, &counters);
	fprintf(stderr, "finish rendering ...\n");
	fprintf(stderr, "FIntegrator::Render used %f seconds.\n", (float)(counters.render_ms / 1000.0));   // integrator.cc:77-79
}

} // namespace jetpbrt
