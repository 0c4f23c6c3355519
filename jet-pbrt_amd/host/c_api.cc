// jet-pbrt_amd/host/c_api.cc -- a procedural C view of the host API (jp_host_*), so that Python harnesses
// (tests, bench.py, __graft_entry__) can build scenes through the SAME call sequence they use on the compiled
// reference (oracle/ref_build/ref_driver.cc: ref_*), i.e. the calls of main.cc:13-111.
#include "jetpbrt.h"
#include "jp_procedural.h"       // jp_procedural_check: what jp_host_texture_procedural accepts

#include <cstring>

using namespace jetpbrt;

namespace
{
struct HostScene
{
	std::shared_ptr<FScene> scene;
	std::vector<std::shared_ptr<FMaterial>> mats;
	std::vector<std::shared_ptr<FTexture>> texs;
	std::vector<std::shared_ptr<FNormalMap>> nmaps;
	FlatScene flat; bool flattened = false;
	std::unique_ptr<FGpuPathIntegrator> integ; int integDepth = -1;
	JpEnvMap envView;                                             // jp_host_flatten_envmap
	std::string error;
};
FColor C3(const float* v) { return FColor(v[0], v[1], v[2]); }
FVector3 V3(const float* v) { return FVector3(v[0], v[1], v[2]); }
void attach(HostScene* hs, const std::shared_ptr<FShape>& shape, int mat, const float* radiance)
{
	std::shared_ptr<FMaterial> m = mat >= 0 ? hs->mats[mat] : nullptr;
	if (radiance) hs->scene->CreateAreaLight(1, C3(radiance), shape, m);
	else hs->scene->CreatePrimitive(shape.get(), m.get(), (const FAreaLight*)nullptr);
}
}

extern "C" {

void* jp_host_scene_new(const char* name) { HostScene* hs = new HostScene; hs->scene = std::make_shared<FScene>(name); return hs; }
void  jp_host_scene_free(void* h) { delete (HostScene*)h; }
const char* jp_host_last_error(void* h) { return ((HostScene*)h)->error.c_str(); }

void jp_host_scene_camera(void* h, const float* lookfrom, const float* front, const float* up, float vfov, float resx, float resy)
{ ((HostScene*)h)->scene->CreateCamera<FCamera>(V3(lookfrom), V3(front), V3(up), vfov, FVector2(resx, resy)); }

int jp_host_scene_envlight(void* h, const float* rgb)
{ HostScene* hs = (HostScene*)h; hs->scene->CreateLight<FEnvironmentLight>(FPoint3(0, 0, 0), 1, C3(rgb)); return hs->scene->LightNum() - 1; }

int jp_host_scene_pointlight(void* h, const float* pos, const float* intensity)
{ HostScene* hs = (HostScene*)h; hs->scene->CreateLight<FPointLight>(V3(pos), 1, C3(intensity)); return hs->scene->LightNum() - 1; }
int jp_host_scene_dirlight(void* h, const float* dir, const float* irradiance)
{ HostScene* hs = (HostScene*)h; hs->scene->CreateLight<FDirectionLight>(FPoint3(0, 0, 0), 1, C3(irradiance), V3(dir)); return hs->scene->LightNum() - 1; }

int jp_host_mat_matte(void* h, const float* rgb) { HostScene* hs = (HostScene*)h; hs->mats.push_back(hs->scene->CreateMaterial<FMatteMaterial>(C3(rgb))); return (int)hs->mats.size() - 1; }
int jp_host_mat_mirror(void* h, const float* rgb) { HostScene* hs = (HostScene*)h; hs->mats.push_back(hs->scene->CreateMaterial<FMirrorMaterial>(C3(rgb))); return (int)hs->mats.size() - 1; }
int jp_host_mat_glass(void* h, float eta, const float* kr, const float* kt) { HostScene* hs = (HostScene*)h; hs->mats.push_back(hs->scene->CreateMaterial<FGlassMaterial>(eta, C3(kr), C3(kt))); return (int)hs->mats.size() - 1; }
int jp_host_mat_plastic(void* h, const float* kd, const float* ks, float rough, int remap) { HostScene* hs = (HostScene*)h; hs->mats.push_back(hs->scene->CreateMaterial<FPlasticMaterial>(C3(kd), C3(ks), rough, remap != 0)); return (int)hs->mats.size() - 1; }
int jp_host_mat_metal(void* h, const float* eta, const float* k, float ur, float vr, int remap) { HostScene* hs = (HostScene*)h; hs->mats.push_back(hs->scene->CreateMaterial<FMetalMaterial>(C3(eta), C3(k), ur, vr, remap != 0)); return (int)hs->mats.size() - 1; }

// textures (FSolidColor / FCheckerTexture / FImageTexture) -> handle index; materials that take one (-1: none)
int jp_host_texture_solid(void* h, const float* rgb) { HostScene* hs = (HostScene*)h; hs->texs.push_back(std::make_shared<FSolidColor>(C3(rgb))); return (int)hs->texs.size() - 1; }
int jp_host_texture_checker(void* h, const float* odd, const float* even) { HostScene* hs = (HostScene*)h; hs->texs.push_back(std::make_shared<FCheckerTexture>(C3(odd), C3(even))); return (int)hs->texs.size() - 1; }
// FProceduralTexture from a JpProcedural (kind not NONE): the texture flattens as the CHECKER of the two colours plus the record
int jp_host_texture_procedural(void* h, const JpProcedural* rec, const float* odd, const float* even)
{
	HostScene* hs = (HostScene*)h;
	if (!rec || rec->kind == JP_PROC_NONE || jp_procedural_check(rec)) { hs->error = std::string("jp_host_texture_procedural: ") + (rec ? jp_procedural_rule(jp_procedural_check(rec)) : "null record"); return -1; }
	auto t = std::make_shared<FProceduralTexture>(rec->kind, C3(odd), C3(even), rec->m, rec->octaves, rec->gain, rec->antialias >= 0, rec->variation, rec->space == JP_PROC_SPACE_UV);
	hs->texs.push_back(t);
	return (int)hs->texs.size() - 1;
}
int jp_host_texture_image(void* h, const unsigned char* rgb8, int w, int hgt) { HostScene* hs = (HostScene*)h; hs->texs.push_back(std::make_shared<FImageTexture>(rgb8, w, hgt)); return (int)hs->texs.size() - 1; }
int jp_host_texture_image_file(void* h, const char* path) { HostScene* hs = (HostScene*)h; hs->texs.push_back(std::make_shared<FImageTexture>(path)); return (int)hs->texs.size() - 1; }
int jp_host_mat_matte_tex(void* h, int tex) { HostScene* hs = (HostScene*)h; if (tex < 0 || tex >= (int)hs->texs.size()) return -1; hs->mats.push_back(hs->scene->CreateMaterial<FMatteMaterial>(hs->texs[tex])); return (int)hs->mats.size() - 1; }
int jp_host_mat_mirror_tex(void* h, int tex) { HostScene* hs = (HostScene*)h; if (tex < 0 || tex >= (int)hs->texs.size()) return -1; hs->mats.push_back(hs->scene->CreateMaterial<FMirrorMaterial>(hs->texs[tex])); return (int)hs->mats.size() - 1; }
int jp_host_mat_plastic_tex(void* h, int tex, const float* ks, float rough, int remap)
{ HostScene* hs = (HostScene*)h; if (tex < 0 || tex >= (int)hs->texs.size()) return -1; hs->mats.push_back(hs->scene->CreateMaterial<FPlasticMaterial>(hs->texs[tex], C3(ks), rough, remap != 0)); return (int)hs->mats.size() - 1; }
// FMaterial::texture of any material (FlattenScene refuses one on glass / metal): 0, or -1 for a bad index
int jp_host_mat_set_texture(void* h, int mat, int tex)
{
	HostScene* hs = (HostScene*)h;
	if (mat < 0 || mat >= (int)hs->mats.size() || tex < -1 || tex >= (int)hs->texs.size()) return -1;
	hs->mats[mat]->texture = tex >= 0 ? hs->texs[tex] : nullptr; hs->flattened = false;
	return 0;
}

int jp_host_scene_mesh(void* h, const char* path, int flip_normal, int flip_handedness, const float* offset, float scale, int mat, const float* radiance)
{
	HostScene* hs = (HostScene*)h;
	std::vector<std::shared_ptr<FShape>> mesh = hs->scene->CreateTriangleMesh(path, flip_normal != 0, flip_handedness != 0, V3(offset), scale);
	std::shared_ptr<FMaterial> m = mat >= 0 ? hs->mats[mat] : nullptr;
	if (radiance) hs->scene->CreateAreaLights(1, C3(radiance), mesh, m);
	else hs->scene->CreatePrimitives(mesh, m);
	return (int)mesh.size();
}

// ... with FSmoothing: smooth_mode 0 flat, 1 the file's vn, 2 computed with the crease angle `angle` (degrees)
int jp_host_scene_mesh_smooth(void* h, const char* path, int flip_normal, int flip_handedness, const float* offset, float scale, int mat, const float* radiance, int smooth_mode, float angle)
{
	HostScene* hs = (HostScene*)h;
	const FSmoothing sm = smooth_mode == FSmoothing::kFile ? FSmoothing::File() : (smooth_mode == FSmoothing::kAngle ? FSmoothing::Angle(angle) : FSmoothing::Flat());
	std::vector<std::shared_ptr<FShape>> mesh = hs->scene->CreateTriangleMesh(path, flip_normal != 0, flip_handedness != 0, V3(offset), scale, sm);
	std::shared_ptr<FMaterial> m = mat >= 0 ? hs->mats[mat] : nullptr;
	if (radiance) hs->scene->CreateAreaLights(1, C3(radiance), mesh, m);
	else hs->scene->CreatePrimitives(mesh, m);
	return (int)mesh.size();
}

void jp_host_scene_rect(void* h, int axis, float a0, float a1, float b0, float b1, float c, int flip, int mat, const float* radiance)
{
	HostScene* hs = (HostScene*)h;
	FRectangle r = axis == 0 ? FRectangle::FromXY(a0, a1, b0, b1, c, flip != 0) : axis == 1 ? FRectangle::FromXZ(a0, a1, b0, b1, c, flip != 0) : FRectangle::FromYZ(a0, a1, b0, b1, c, flip != 0);
	attach(hs, hs->scene->CreateShape<FRectangle>(r), mat, radiance);
}

void jp_host_scene_sphere(void* h, const float* center, float radius, int mat, const float* radiance)
{ HostScene* hs = (HostScene*)h; attach(hs, hs->scene->CreateShape<FSphere>(V3(center), radius), mat, radiance); }

void jp_host_scene_disk(void* h, const float* pos, const float* normal, float radius, int mat, const float* radiance)
{ HostScene* hs = (HostScene*)h; attach(hs, hs->scene->CreateShape<FDisk>(V3(pos), V3(normal), radius), mat, radiance); }

void jp_host_scene_set_reference_tree(void* h, int on) { ((HostScene*)h)->scene->referenceTree = on != 0; ((HostScene*)h)->scene->certifiedWalk = on == 2; }   // 1: verbatim walk, 2: certified walk
void jp_host_scene_set_device_build(void* h, int on) { ((HostScene*)h)->scene->deviceBuild = on != 0; ((HostScene*)h)->scene->hostBuild = on == 0; }   // explicit either way
void jp_host_scene_set_light_sampling(void* h, int mode) { ((HostScene*)h)->scene->SetLightSampling(mode); }   // FScene::SetLightSampling (JP_LIGHTS_*)
void jp_host_scene_set_estimator(void* h, int mode) { ((HostScene*)h)->scene->SetEstimator(mode); }   // FScene::SetEstimator (JP_ESTIMATOR_*)
// FCamera::SetLens / FocusAt on the scene's camera (radius 0: the pinhole again; focus_at != 0: focus on what film position (fx, fy) sees); -1 without a camera.
// jp_host_last_focus: FCamera::LastFocus, the focus distance of the last render with a lens
int jp_host_scene_set_lens(void* h, float radius, float focus, int blades, float rotation, int focus_at, float fx, float fy)
{
	HostScene* hs = (HostScene*)h;
	if (!hs->scene->camera) { hs->error = "jp_host_scene_set_lens: the scene has no camera"; return -1; }
	hs->scene->camera->SetLens(radius, focus, blades, rotation);
	if (focus_at) hs->scene->camera->FocusAt(fx, fy);
	return 0;
}
// FCamera::SetProjection on the scene's camera (kind 0: the pinhole again), after FCamera::CheckProjection -- the library's jp_check_projection; the camera keeps
// the projection it had when that refuses.  0, or -1 with jp_host_last_error set (no camera; the check's message)
int jp_host_scene_set_projection(void* h, int kind, float ortho_scale, float fov_deg, int fit)
{
	HostScene* hs = (HostScene*)h;
	if (!hs->scene->camera) { hs->error = "jp_host_scene_set_projection: the scene has no camera"; return -1; }
	FCamera& cam = *hs->scene->camera;
	const int k0 = cam.projKind, f0 = cam.projFit; const Float s0 = cam.projOrthoScale, v0 = cam.projFovDeg;
	cam.SetProjection(kind, ortho_scale, fov_deg, fit);
	std::string msg;
	if (!cam.CheckProjection(&msg)) { cam.SetProjection(k0, s0, v0, f0); hs->error = msg; return -1; }
	return 0;
}
float jp_host_last_focus(void* h) { HostScene* hs = (HostScene*)h; return hs->scene->camera ? hs->scene->camera->LastFocus() : 0.f; }
// FScene::SetEnvironmentMap from memory (3 * w * hgt floats, top row first; null: no map) or from a file (FEnvironmentMap::FromFile); importance -1:
// the A/B hook of JpEnvMap.  0, or -1 with jp_host_last_error set
int jp_host_scene_envmap(void* h, const float* rgb, int w, int hgt, int up_axis, int importance)
{
	HostScene* hs = (HostScene*)h;
	if (!rgb) { hs->scene->SetEnvironmentMap(nullptr); return 0; }
	auto m = std::make_shared<FEnvironmentMap>(rgb, w, hgt);
	if (!m->Valid()) { hs->error = "jp_host_scene_envmap: size out of range (1 .. 4096 per side)"; return -1; }
	if (up_axis != JP_ENV_UP_Z && up_axis != JP_ENV_UP_Y) { hs->error = "jp_host_scene_envmap: unknown up axis"; return -1; }
	hs->scene->SetEnvironmentMap(m, up_axis); hs->scene->environmentImportance = importance;
	return 0;
}
int jp_host_scene_envmap_file(void* h, const char* path, int up_axis)
{
	HostScene* hs = (HostScene*)h;
	std::string err;
	auto m = FEnvironmentMap::FromFile(path, &err);
	if (!m) { hs->error = std::string("jp_host_scene_envmap_file: ") + (path ? path : "") + ": " + err; return -1; }
	if (up_axis != JP_ENV_UP_Z && up_axis != JP_ENV_UP_Y) { hs->error = "jp_host_scene_envmap_file: unknown up axis"; return -1; }
	hs->scene->SetEnvironmentMap(m, up_axis); hs->scene->environmentImportance = 0;
	return 0;
}
// the scene's map as the JpEnvMap FGpuPathIntegrator::Render hands to jp_set_environment_map (owned by the handle; null: no map)
const JpEnvMap* jp_host_flatten_envmap(void* h)
{
	HostScene* hs = (HostScene*)h;
	const FEnvironmentMap* m = hs->scene->environmentMap.get();
	if (!m || !m->Valid()) return nullptr;
	JpEnvMap& v = hs->envView;
	v.struct_bytes = (int32_t)sizeof(JpEnvMap); v.width = m->width; v.height = m->height; v.up_axis = hs->scene->environmentUp; v.importance = hs->scene->environmentImportance; v.rgb = m->data.data();
	return &v;
}

// normal maps (FNormalMap) -> handle index, -1 with jp_host_last_error set: from RGB8 memory, from a file, from a grey height map
static int add_normal_map(HostScene* hs, const std::shared_ptr<FNormalMap>& m, const char* who)
{
	if (!m || !m->Valid()) { hs->error = std::string(who) + ": no image, or a size out of range (1 .. 16384 per side)"; return -1; }
	hs->nmaps.push_back(m); return (int)hs->nmaps.size() - 1;
}
int jp_host_normal_map(void* h, const unsigned char* rgb8, int w, int hgt) { return add_normal_map((HostScene*)h, std::make_shared<FNormalMap>(rgb8, w, hgt), "jp_host_normal_map"); }
int jp_host_normal_map_file(void* h, const char* path) { return add_normal_map((HostScene*)h, FNormalMap::FromFile(path), "jp_host_normal_map_file"); }
int jp_host_normal_map_from_procedural(void* h, const JpProcedural* rec, int w, int hgt, float scale)
{
	std::shared_ptr<FNormalMap> m = rec ? FNormalMap::FromProcedural(*rec, w, hgt, scale) : nullptr;
	if (!m) { ((HostScene*)h)->error = "jp_host_normal_map_from_procedural: a record the validation refuses, or a size out of range"; return -1; }
	return add_normal_map((HostScene*)h, m, "jp_host_normal_map_from_procedural");
}
int jp_host_normal_map_from_height(void* h, const unsigned char* grey, int w, int hgt, float scale) { return add_normal_map((HostScene*)h, FNormalMap::FromHeight(grey, w, hgt, scale), "jp_host_normal_map_from_height"); }
// the map's size (either pointer may be null) and, with rgb8_out, its 3 * w * hgt bytes
int jp_host_normal_map_read(void* h, int map, int* w, int* hgt, unsigned char* rgb8_out)
{
	HostScene* hs = (HostScene*)h;
	if (map < 0 || map >= (int)hs->nmaps.size()) { hs->error = "jp_host_normal_map_read: no such map"; return -1; }
	const FNormalMap& m = *hs->nmaps[map];
	if (w) *w = m.width;
	if (hgt) *hgt = m.height;
	if (rgb8_out) std::memcpy(rgb8_out, m.data.data(), m.data.size());
	return 0;
}
// FMaterial::normalMap / normalStrength of any material (map -1: none)
int jp_host_mat_set_normal_map(void* h, int mat, int map, float strength)
{
	HostScene* hs = (HostScene*)h;
	if (mat < 0 || mat >= (int)hs->mats.size() || map < -1 || map >= (int)hs->nmaps.size()) { hs->error = "jp_host_mat_set_normal_map: no such material or map"; return -1; }
	hs->mats[mat]->normalMap = map >= 0 ? hs->nmaps[map] : nullptr; hs->mats[mat]->normalStrength = strength; hs->flattened = false;
	return 0;
}

// texture sampling: FImageTexture::SetSampling / FNormalMap::SetSampling / FScene::SetTextureSamplingDefault from a JpTexSampler (null: back to none of its own)
static FTexSampling sampling_of(const JpTexSampler* r)
{
	FTexSampling s; s.wrapU = (EWrap)r->wrap_u; s.wrapV = (EWrap)r->wrap_v; s.filter = (EFilter)r->filter;
	s.scaleU = r->scale_u; s.scaleV = r->scale_v; s.offsetU = r->offset_u; s.offsetV = r->offset_v;
	return s;
}
int jp_host_texture_set_sampling(void* h, int tex, const JpTexSampler* r)
{
	HostScene* hs = (HostScene*)h;
	FImageTexture* it = tex >= 0 && tex < (int)hs->texs.size() ? dynamic_cast<FImageTexture*>(hs->texs[tex].get()) : nullptr;
	if (!it) { hs->error = "jp_host_texture_set_sampling: no such image texture"; return -1; }
	if (r) it->SetSampling(sampling_of(r)); else { it->sampling = FTexSampling(); it->hasSampling = false; }
	hs->flattened = false;
	return 0;
}
int jp_host_normal_map_set_sampling(void* h, int map, const JpTexSampler* r)
{
	HostScene* hs = (HostScene*)h;
	if (map < 0 || map >= (int)hs->nmaps.size()) { hs->error = "jp_host_normal_map_set_sampling: no such map"; return -1; }
	if (r) hs->nmaps[map]->SetSampling(sampling_of(r)); else { hs->nmaps[map]->sampling = FTexSampling(); hs->nmaps[map]->hasSampling = false; }
	hs->flattened = false;
	return 0;
}
int jp_host_scene_set_texture_sampling_default(void* h, const JpTexSampler* r)
{
	HostScene* hs = (HostScene*)h;
	if (r) hs->scene->SetTextureSamplingDefault(sampling_of(r)); else { hs->scene->textureSamplingDefault = FTexSampling(); hs->scene->hasTextureSamplingDefault = false; }
	hs->flattened = false;
	return 0;
}
// mip maps: FImageTexture::SetMipmaps (on < 0: back to the scene's default) and FScene::SetTextureMipmapDefault with the scene's footprint scale and bounce spread
int jp_host_texture_set_mipmaps(void* h, int tex, int on)
{
	HostScene* hs = (HostScene*)h;
	FImageTexture* it = tex >= 0 && tex < (int)hs->texs.size() ? dynamic_cast<FImageTexture*>(hs->texs[tex].get()) : nullptr;
	if (!it) { hs->error = "jp_host_texture_set_mipmaps: no such image texture"; return -1; }
	if (on >= 0) it->SetMipmaps(on != 0); else { it->mipmaps = false; it->hasMipmaps = false; }
	hs->flattened = false;
	return 0;
}
int jp_host_scene_set_texture_mipmap_default(void* h, int on, float footprint_scale, float bounce_spread)
{
	HostScene* hs = (HostScene*)h;
	hs->scene->SetTextureMipmapDefault(on != 0); hs->scene->mipFootprintScale = footprint_scale; hs->scene->mipBounceSpread = bounce_spread;
	hs->flattened = false;
	return 0;
}
void jp_host_scene_preprocess(void* h) { HostScene* hs = (HostScene*)h; hs->scene->Preprocess(); hs->flattened = false; }
int  jp_host_num_primitives(void* h) { return (int)((HostScene*)h)->scene->primitives.size(); }
int  jp_host_num_lights(void* h) { return ((HostScene*)h)->scene->LightNum(); }

// the flattened SoA view (owned by the handle; valid until the next preprocess/free)
const JpScene* jp_host_flatten(void* h)
{
	HostScene* hs = (HostScene*)h;
	if (!hs->flattened) { if (!FlattenScene(*hs->scene, hs->flat, &hs->error)) return nullptr; hs->flattened = true; }
	return &hs->flat.view;
}

// the flattened textures (valid with jp_host_flatten's view; n_textures 0 for a scene without a textured material)
const JpTextures* jp_host_flatten_textures(void* h)
{
	HostScene* hs = (HostScene*)h;
	if (!jp_host_flatten(h)) return nullptr;
	return &hs->flat.textures;
}

// the flattened vertex normals (valid with jp_host_flatten's view; null: the scene has no smooth triangle, or the flattening failed)
const JpVertexNormals* jp_host_flatten_normals(void* h)
{
	HostScene* hs = (HostScene*)h;
	if (!jp_host_flatten(h) || hs->flat.n_smooth == 0) return nullptr;
	return &hs->flat.normals;
}

// the flattened normal maps (valid with jp_host_flatten's view; null: no material carries a map, or the flattening failed)
const JpNormalMaps* jp_host_flatten_normal_maps(void* h)
{
	HostScene* hs = (HostScene*)h;
	if (!jp_host_flatten(h) || hs->flat.n_normal_mapped == 0) return nullptr;
	return &hs->flat.normalMaps;
}

// the flattened sampling records (valid with jp_host_flatten's view; null: every record is the identity, or the flattening failed)
const JpTextureSampling* jp_host_flatten_texture_sampling(void* h)
{
	HostScene* hs = (HostScene*)h;
	if (!jp_host_flatten(h) || hs->flat.n_sampled == 0) return nullptr;
	return &hs->flat.sampling;
}

// the flattened procedural records (valid with jp_host_flatten's view; null: every kind is NONE, or the flattening failed)
const JpTextureProcedurals* jp_host_flatten_texture_procedurals(void* h)
{
	HostScene* hs = (HostScene*)h;
	if (!jp_host_flatten(h) || hs->flat.n_procedural == 0) return nullptr;
	return &hs->flat.procedurals;
}

// the flattened mipmap modes (valid with jp_host_flatten's view; null: every mode is OFF, or the flattening failed)
const JpTextureMipmaps* jp_host_flatten_texture_mipmaps(void* h)
{
	HostScene* hs = (HostScene*)h;
	if (!jp_host_flatten(h) || hs->flat.n_mipmapped == 0) return nullptr;
	return &hs->flat.mipmaps;
}

// FGpuPathIntegrator(maxdepth).Render(scene, FCounterSampler(spp, seed), film, numthreads) -> rgb (added onto zeros)
int jp_host_render(void* h, int W, int H, int spp, int maxdepth, unsigned seed, int device, int shard_index, int shard_count, float* film_out, JpCounters* counters)
{
	HostScene* hs = (HostScene*)h;
	if (!hs->integ || hs->integDepth != maxdepth) { hs->integ.reset(new FGpuPathIntegrator(maxdepth, device)); hs->integDepth = maxdepth; }
	hs->integ->SetShard(shard_index, shard_count > 0 ? shard_count : 1);
	FFilm film(W, H);
	FCounterSampler sampler(spp, seed);
	hs->integ->Render(hs->scene.get(), &sampler, &film, 16);
	if (hs->integ->LastStatus() != JP_OK) return hs->integ->LastStatus();
	for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const FColor& c = static_cast<const FFilm&>(film)(x, y); float* o = film_out + 3 * ((size_t)y * W + x); o[0] = c.r; o[1] = c.g; o[2] = c.b; }
	if (counters) *counters = hs->integ->Counters();
	return JP_OK;
}

// FWhittedIntegrator(maxdepth) (kind 1) / FDebugIntegrator (kind 2) .Render(scene, FCounterSampler(spp, seed), film, numthreads)
int jp_host_render_other(void* h, int kind, int W, int H, int spp, int maxdepth, unsigned seed, int device, float* film_out)
{
	HostScene* hs = (HostScene*)h;
	std::unique_ptr<FGpuPathIntegrator> integ;
	if (kind == JP_INTEGRATOR_WHITTED) integ.reset(new FWhittedIntegrator(maxdepth, device)); else integ.reset(new FDebugIntegrator(device));
	FFilm film(W, H);
	FCounterSampler sampler(spp, seed);
	integ->Render(hs->scene.get(), &sampler, &film, 16);
	if (integ->LastStatus() != JP_OK) return integ->LastStatus();
	for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const FColor& c = static_cast<const FFilm&>(film)(x, y); float* o = film_out + 3 * ((size_t)y * W + x); o[0] = c.r; o[1] = c.g; o[2] = c.b; }
	return JP_OK;
}

// The film output path with the tone map on the device: FFilm::RequestDeviceLDR(ldr_only) -> Render -> the 8-bit pixels (and,
// unless ldr_only, the fp32 film) -> optionally FFilm::SaveAsImage(filename, type).  rgb8_out: W*H*3 bytes; film_out may be null.
int jp_host_render_ldr(void* h, int W, int H, int spp, int maxdepth, unsigned seed, int device, int ldr_only, unsigned char* rgb8_out, float* film_out, const char* filename, int type)
{
	HostScene* hs = (HostScene*)h;
	if (ldr_only && ((filename && filename[0] && type == 2) || film_out)) return JP_ERR_INVALID_ARGUMENT;   // an LDR-only film has no fp32 pixels for an .hdr file or a float buffer
	if (!hs->integ || hs->integDepth != maxdepth) { hs->integ.reset(new FGpuPathIntegrator(maxdepth, device)); hs->integDepth = maxdepth; }
	hs->integ->SetShard(0, 1);
	FFilm film(W, H);
	film.RequestDeviceLDR(ldr_only != 0);
	FCounterSampler sampler(spp, seed);
	hs->integ->Render(hs->scene.get(), &sampler, &film, 16);
	if (hs->integ->LastStatus() != JP_OK) return hs->integ->LastStatus();
	if (!film.HasLDR()) return JP_ERR_DEVICE;
	if (rgb8_out) std::memcpy(rgb8_out, film.ldr8.data(), film.ldr8.size());
	if (film_out) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const FColor& c = static_cast<const FFilm&>(film)(x, y); float* o = film_out + 3 * ((size_t)y * W + x); o[0] = c.r; o[1] = c.g; o[2] = c.b; }
	if (filename && filename[0]) return film.SaveAsImage(filename, type == 0 ? EImageType::PPM : (type == 2 ? EImageType::HDR : EImageType::BMP)) ? JP_OK : JP_ERR_INVALID_ARGUMENT;
	return JP_OK;
}

// FFilm::RequestGuides(guide_spp) (denoise 0) / RequestDenoise(guide_spp) (denoise 1) [+ RequestDeviceLDR(ldr == 2): ldr 0 none, 1 next to the fp32 film,
// 2 instead of it] -> Render -> the film (denoised when asked for), the guides and the 8-bit pixels; any output may be null
int jp_host_render_denoised(void* h, int W, int H, int spp, int maxdepth, unsigned seed, int device, int guide_spp, int denoise, int ldr,
                            float* film_out, float* albedo_out, float* normal_out, float* depth_out, unsigned char* rgb8_out)
{
	HostScene* hs = (HostScene*)h;
	if (ldr == 2 && film_out) return JP_ERR_INVALID_ARGUMENT;
	if (!hs->integ || hs->integDepth != maxdepth) { hs->integ.reset(new FGpuPathIntegrator(maxdepth, device)); hs->integDepth = maxdepth; }
	hs->integ->SetShard(0, 1);
	FFilm film(W, H);
	if (denoise) film.RequestDenoise(guide_spp); else film.RequestGuides(guide_spp);
	if (ldr) film.RequestDeviceLDR(ldr == 2);
	FCounterSampler sampler(spp, seed);
	hs->integ->Render(hs->scene.get(), &sampler, &film, 16);
	if (hs->integ->LastStatus() != JP_OK) return hs->integ->LastStatus();
	const size_t n = (size_t)W * H;
	if (film.Albedo().size() != n || film.Normal().size() != n || film.Depth().size() != n || (ldr && !film.HasLDR())) return JP_ERR_DEVICE;
	if (film_out) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const FColor& c = static_cast<const FFilm&>(film)(x, y); float* o = film_out + 3 * ((size_t)y * W + x); o[0] = c.r; o[1] = c.g; o[2] = c.b; }
	for (size_t i = 0; i < n; i++)
	{
		if (albedo_out) { albedo_out[3 * i] = film.Albedo()[i].r; albedo_out[3 * i + 1] = film.Albedo()[i].g; albedo_out[3 * i + 2] = film.Albedo()[i].b; }
		if (normal_out) { normal_out[3 * i] = film.Normal()[i].x; normal_out[3 * i + 1] = film.Normal()[i].y; normal_out[3 * i + 2] = film.Normal()[i].z; }
		if (depth_out) depth_out[i] = film.Depth()[i];
	}
	if (rgb8_out && ldr) std::memcpy(rgb8_out, film.ldr8.data(), film.ldr8.size());
	return JP_OK;
}

// FFilm::RequestVariance() (variance 1) and / or RequestGuides(guide_spp) (guide_spp > 0, denoise 0) / RequestDenoise(guide_spp, { varianceGuided }) (denoise 1) [+ SetHDR] -> Render -> the
// film, the variance plane and the guides; any output may be null
int jp_host_render_variance(void* h, int W, int H, int spp, int maxdepth, unsigned seed, int device, int variance, int guide_spp, int denoise, int hdr,
                            float* film_out, float* variance_out, float* albedo_out, float* normal_out, float* depth_out)
{
	HostScene* hs = (HostScene*)h;
	if (!hs->integ || hs->integDepth != maxdepth) { hs->integ.reset(new FGpuPathIntegrator(maxdepth, device)); hs->integDepth = maxdepth; }
	hs->integ->SetShard(0, 1);
	FFilm film(W, H);
	if (hdr) film.SetHDR();
	if (variance) film.RequestVariance();
	if (denoise) { FDenoiseOptions o; o.varianceGuided = true; film.RequestDenoise(guide_spp, o); } else if (guide_spp > 0) film.RequestGuides(guide_spp);
	FCounterSampler sampler(spp, seed);
	hs->integ->Render(hs->scene.get(), &sampler, &film, 16);
	if (hs->integ->LastStatus() != JP_OK) return hs->integ->LastStatus();
	const size_t n = (size_t)W * H;
	const bool guides = denoise || guide_spp > 0;
	if ((variance || denoise) && film.Variance().size() != n) return JP_ERR_DEVICE;
	if (guides && (film.Albedo().size() != n || film.Normal().size() != n || film.Depth().size() != n)) return JP_ERR_DEVICE;
	if (film_out) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const FColor& c = static_cast<const FFilm&>(film)(x, y); float* o = film_out + 3 * ((size_t)y * W + x); o[0] = c.r; o[1] = c.g; o[2] = c.b; }
	if (variance_out && film.Variance().size() == n) std::memcpy(variance_out, film.Variance().data(), n * sizeof(float));
	for (size_t i = 0; guides && i < n; i++)
	{
		if (albedo_out) { albedo_out[3 * i] = film.Albedo()[i].r; albedo_out[3 * i + 1] = film.Albedo()[i].g; albedo_out[3 * i + 2] = film.Albedo()[i].b; }
		if (normal_out) { normal_out[3 * i] = film.Normal()[i].x; normal_out[3 * i + 1] = film.Normal()[i].y; normal_out[3 * i + 2] = film.Normal()[i].z; }
		if (depth_out) depth_out[i] = film.Depth()[i];
	}
	return JP_OK;
}

// FFilm::SetAdaptive(threshold, min_spp, step_spp, dilate) [+ SetHDR, RequestGuides(guide_spp) / RequestDenoise(guide_spp, { varianceGuided })] -> Render (spp: the most a pixel
// takes) -> the film, FFilm::SampleCounts() and FFilm::Variance(); any output may be null
int jp_host_render_adaptive(void* h, int W, int H, int spp, int maxdepth, unsigned seed, int device, float threshold, int min_spp, int step_spp, int dilate, int guide_spp, int denoise, int hdr,
                            float* film_out, int32_t* counts_out, float* variance_out)
{
	HostScene* hs = (HostScene*)h;
	if (!hs->integ || hs->integDepth != maxdepth) { hs->integ.reset(new FGpuPathIntegrator(maxdepth, device)); hs->integDepth = maxdepth; }
	hs->integ->SetShard(0, 1);
	FFilm film(W, H);
	if (hdr) film.SetHDR();
	film.SetAdaptive(threshold, min_spp, step_spp, dilate != 0);
	if (denoise) { FDenoiseOptions o; o.varianceGuided = true; film.RequestDenoise(guide_spp, o); } else if (guide_spp > 0) film.RequestGuides(guide_spp);
	FCounterSampler sampler(spp, seed);
	hs->integ->Render(hs->scene.get(), &sampler, &film, 16);
	if (hs->integ->LastStatus() != JP_OK) return hs->integ->LastStatus();
	const size_t n = (size_t)W * H;
	if (film.SampleCounts().size() != n || film.Variance().size() != n) return JP_ERR_DEVICE;
	if (film_out) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const FColor& c = static_cast<const FFilm&>(film)(x, y); float* o = film_out + 3 * ((size_t)y * W + x); o[0] = c.r; o[1] = c.g; o[2] = c.b; }
	if (counts_out) std::memcpy(counts_out, film.SampleCounts().data(), n * sizeof(int32_t));
	if (variance_out) std::memcpy(variance_out, film.Variance().data(), n * sizeof(float));
	return JP_OK;
}

// The linear-light film: FFilm::SetHDR(hdr) / SetSampleClamp(sample_clamp) / SetToneMap(curve, auto_exposure, ev, white) when tonemap != 0 [+ RequestDeviceLDR(true) when
// ldr_only] -> Render -> the fp32 film (unless ldr_only), the 8-bit pixels (with a tone map or ldr_only), FFilm::ToneMapScale() -> optionally SaveAsImage(filename, type).
// Any output may be null.
int jp_host_render_film(void* h, int W, int H, int spp, int maxdepth, unsigned seed, int device, int hdr, float sample_clamp, int tonemap, int curve, int auto_exposure, float ev, float white,
                        int ldr_only, float* film_out, unsigned char* rgb8_out, float* scale_out, const char* filename, int type)
{
	HostScene* hs = (HostScene*)h;
	if (ldr_only && ((filename && filename[0] && type == 2) || film_out)) return JP_ERR_INVALID_ARGUMENT;   // an LDR-only film has no fp32 pixels for an .hdr file or a float buffer
	if (!hs->integ || hs->integDepth != maxdepth) { hs->integ.reset(new FGpuPathIntegrator(maxdepth, device)); hs->integDepth = maxdepth; }
	hs->integ->SetShard(0, 1);
	FFilm film(W, H);
	if (hdr) film.SetHDR();
	if (sample_clamp != 0) film.SetSampleClamp(sample_clamp);
	if (tonemap) { FToneMap t; t.curve = curve; t.autoExposure = auto_exposure != 0; t.ev = ev; t.white = white; film.SetToneMap(t); }
	if (ldr_only) film.RequestDeviceLDR(true);
	FCounterSampler sampler(spp, seed);
	hs->integ->Render(hs->scene.get(), &sampler, &film, 16);
	if (hs->integ->LastStatus() != JP_OK) return hs->integ->LastStatus();
	if ((tonemap || ldr_only) && !film.HasLDR()) return JP_ERR_DEVICE;
	if (rgb8_out && film.HasLDR()) std::memcpy(rgb8_out, film.ldr8.data(), film.ldr8.size());
	if (film_out) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const FColor& c = static_cast<const FFilm&>(film)(x, y); float* o = film_out + 3 * ((size_t)y * W + x); o[0] = c.r; o[1] = c.g; o[2] = c.b; }
	if (scale_out) *scale_out = film.ToneMapScale();
	if (filename && filename[0]) return film.SaveAsImage(filename, type == 0 ? EImageType::PPM : (type == 2 ? EImageType::HDR : EImageType::BMP)) ? JP_OK : JP_ERR_INVALID_ARGUMENT;
	return JP_OK;
}

// The reference's reflection classes by name (jetpbrt.h "reflection API"): builds the named class the way reference code would and
// calls Evalf / Pdf / Sample once.  which: 0 FPhongSpecularReflection(Ks, exponent), 1 FMicrofacetReflection(R, Beckmann(ax, ay, vis),
// FresnelNoOp), 2 FMicrofacetTransmission(T, TrowbridgeReitz(ax, ay, vis), etaA, etaB).  out: f[3], pdf, sample f[3], wi[3], pdf, flags
int jp_host_bsdf_class(int which, const float* color, float p0, float p1, int vis, float etaA, float etaB, const float* n, const float* wo, const float* wi, const float* u, float* out)
{
	FFrame frame(FVector3(n[0], n[1], n[2]));
	std::unique_ptr<FBSDF> b;
	const FColor c(color[0], color[1], color[2]);
	if (which == 0) b.reset(new FPhongSpecularReflection(frame, c, p0));
	else if (which == 1) b.reset(new FMicrofacetReflection(frame, c, new BeckmannDistribution(p0, p1, vis != 0), new FresnelNoOp()));
	else if (which == 2) b.reset(new FMicrofacetTransmission(frame, c, new TrowbridgeReitzDistribution(p0, p1, vis != 0), etaA, etaB));
	else return JP_ERR_INVALID_ARGUMENT;
	const FVector3 a(wo[0], wo[1], wo[2]), d(wi[0], wi[1], wi[2]);
	FColor f = b->Evalf(a, d); Float pdf = b->Pdf(a, d); FBSDFSample s = b->Sample(a, FVector2(u[0], u[1]));
	out[0] = f.r; out[1] = f.g; out[2] = f.b; out[3] = pdf; out[4] = s.f.r; out[5] = s.f.g; out[6] = s.f.b; out[7] = s.wi.x; out[8] = s.wi.y; out[9] = s.wi.z; out[10] = s.pdf; out[11] = (float)s.ebsdf;
	return JP_OK;
}

// FGpuPathIntegrator::Render with one of the reference's other samplers: 0 FRandomSampler, 1 FStratifiedSampler, 2 FDebugSampler
int jp_host_render_sampler(void* h, int sampler, int W, int H, int spp, int maxdepth, int device, float* film_out)
{
	HostScene* hs = (HostScene*)h;
	FGpuPathIntegrator integ(maxdepth, device);
	FFilm film(W, H);
	std::unique_ptr<FSampler> s;
	if (sampler == 2) s.reset(new FDebugSampler(spp)); else if (sampler == 1) s.reset(new FStratifiedSampler(spp)); else s.reset(new FRandomSampler(spp));
	integ.Render(hs->scene.get(), s.get(), &film, 16);
	if (integ.LastStatus() != JP_OK) return integ.LastStatus();
	for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const FColor& c = static_cast<const FFilm&>(film)(x, y); float* o = film_out + 3 * ((size_t)y * W + x); o[0] = c.r; o[1] = c.g; o[2] = c.b; }
	return JP_OK;
}

// gamma_encoding (film.h:24) on the host for n values (tests: the device's bytes must equal these)
void jp_host_gamma_encode(const float* x, int n, unsigned char* out) { for (int i = 0; i < n; i++) out[i] = gamma_encoding(x[i]); }

// FFilm::SaveAsImage on an rgb buffer (type 0 PPM, 1 BMP, 2 HDR): returns 1 on success
int jp_host_save_image(const float* rgb, int W, int H, const char* filename, int type)
{
	FFilm film(W, H);
	for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) { const float* p = rgb + 3 * ((size_t)y * W + x); film(x, y) = FColor(p[0], p[1], p[2]); }
	return film.SaveAsImage(filename, type == 0 ? EImageType::PPM : (type == 2 ? EImageType::HDR : EImageType::BMP)) ? 1 : 0;
}

} // extern "C"
