// jet-pbrt_amd/host/jetpbrt.h -- host-side mirror of the reference's Scene/Camera/Film/Sampler/Material/
// Integrator API vocabulary (SURVEY.md section 7 "design stance"), written from scratch for the GPU path:
// objects here only DESCRIBE a scene; nothing in this layer traces a ray.  FScene::Preprocess() builds the
// BVH, FlattenScene() turns the preprocessed scene into the SoA arrays of include/jetpbrt_amd.h, and
// FGpuPathIntegrator::Render() -- same signature as FIntegrator::Render (integrator.h:32) -- hands them to
// the HIP library through the C ABI.
//
// Names follow the reference so that code written against it (main.cc:13-111) ports by changing the
// namespace.  Unlike the reference objects (whose parameters are protected), every
// object exposes the state the flattener needs.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "jetpbrt_amd.h"

namespace jetpbrt
{
typedef float Float;                                             // pbrt.h:27
constexpr Float kPi = (Float)3.14159265358979323846;             // pbrt.h:39

struct FColor                                                    // color.h:13-69 (data + what the host needs)
{
	Float r, g, b;
	FColor() : r(0), g(0), b(0) {}
	FColor(Float v) : r(v), g(v), b(v) {}
	FColor(Float rr, Float gg, Float bb) : r(rr), g(gg), b(bb) {}
	FColor operator-(const FColor& c) const { return FColor(r - c.r, g - c.g, b - c.b); }
	Float Luminance() const { return 0.212671f * r + 0.715160f * g + 0.072169f * b; }   // color.h:45-48
};

struct FVector2 { Float x, y; FVector2() : x(0), y(0) {} FVector2(Float vx, Float vy) : x(vx), y(vy) {} };
typedef FVector2 FPoint2;

struct FVector3                                                  // geometry.h:65-159
{
	Float x, y, z;
	FVector3() : x(0), y(0), z(0) {}
	FVector3(Float vx, Float vy, Float vz) : x(vx), y(vy), z(vz) {}
	FVector3 operator-() const { return FVector3(-x, -y, -z); }
	FVector3 operator+(const FVector3& v) const { return FVector3(x + v.x, y + v.y, z + v.z); }
	FVector3 operator-(const FVector3& v) const { return FVector3(x - v.x, y - v.y, z - v.z); }
	FVector3 operator*(Float s) const { return FVector3(x * s, y * s, z * s); }
	FVector3 operator/(Float s) const { return FVector3(x / s, y / s, z / s); }
	Float Length2() const { return x * x + y * y + z * z; }
	Float Length() const { return std::sqrt(Length2()); }
	FVector3 Normalize() const { return *this / Length(); }
	FVector3 Cross(const FVector3& v) const { return FVector3(y * v.z - z * v.y, z * v.x - x * v.z, x * v.y - y * v.x); }
	Float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
};
typedef FVector3 FPoint3;
typedef FVector3 FNormal3;
inline FVector3 Normalize(const FVector3& v) { return v.Normalize(); }
inline FVector3 Cross(const FVector3& a, const FVector3& b) { return a.Cross(b); }

// axis-aligned box with the reference's semantics (geometry.h:244-315): needed bit-for-bit because the
// environment light's worldRadius (light.cc:26-33) is derived from the union of the shape bounds.
struct FBounds3
{
	FPoint3 _min, _max;
	FBounds3();
	FBounds3(const FPoint3& p1, const FPoint3& p2);
	void Expand(const FBounds3& b);
	FBounds3 Join(const FPoint3& p) const;
	void CheckThinness(Float thinness = 0.01f);
	void BoundingSphere(FPoint3& center, Float& radius) const;
};

// ---- shapes (geometry only; intersection lives on the device) -----------------------------------------------
class FShape
{
public:
	virtual ~FShape() = default;
	virtual int Kind() const = 0;                                // JP_SHAPE_*
	const FBounds3& WorldBounds() const { return worldBox; }
	FBounds3 worldBox;          // the reference's bounds (thin boxes padded by 0.01, geometry.h:299-304): world bound / env radius
	FBounds3 tightBox;          // exact extent: what our own BVH is built over (padding happens at upload, relative)
};

class FTriangle : public FShape                                  // shape.h:277-369
{
public:
	FTriangle(const FPoint3& p0, const FPoint3& p1, const FPoint3& p2, bool flip_normal = false);
	FTriangle(const FPoint3& p0, const FPoint3& p1, const FPoint3& p2, const FPoint2& uv0, const FPoint2& uv1, const FPoint2& uv2, bool flip_normal = false);   // shape.h:280
	int Kind() const override { return JP_SHAPE_TRIANGLE; }
	FPoint3 p0, p1, p2; FNormal3 normal;
	FPoint2 uv0, uv1, uv2;                                       // texture coordinates of the vertices (0 unless given)
	// unit vertex normals (INTEGRATION.md "Vertex normals"): shading interpolates them when `smooth`; a flat triangle (the default) shades with `normal`
	FNormal3 n0, n1, n2; bool smooth = false;
	void SetVertexNormals(const FNormal3& a, const FNormal3& b, const FNormal3& c) { n0 = a; n1 = b; n2 = c; smooth = true; }
};

// How a mesh gets vertex normals: flat (the default -- as ever, even when the file has `vn`), the file's `vn` where a face carries them, or computed:
// corner k of triangle T at OBJ position index v gets normalize(sum of angle_U(v) * Ng_U) over the triangles U sharing v with dot(Ng_T, Ng_U) >= cos(angle),
// T itself always; accumulated in double, in face order; a zero sum gives Ng_T.
struct FSmoothing
{
	enum { kFlat = 0, kFile = 1, kAngle = 2 };
	int mode = kFlat; Float angle = 0;
	static FSmoothing Flat() { return FSmoothing(); }
	static FSmoothing File() { FSmoothing s; s.mode = kFile; return s; }
	static FSmoothing Angle(Float degrees) { FSmoothing s; s.mode = kAngle; s.angle = degrees; return s; }
};

class FRectangle : public FShape                                 // shape.h:380-472, shape.cc:76-95
{
public:
	FRectangle(const FPoint3& p0, const FPoint3& p1, const FPoint3& p2, const FPoint3& p3, bool flip_normal = false);
	static FRectangle FromXY(Float x0, Float x1, Float y0, Float y1, Float z, bool flip_normal = false);
	static FRectangle FromXZ(Float x0, Float x1, Float z0, Float z1, Float y, bool flip_normal = false);
	static FRectangle FromYZ(Float y0, Float y1, Float z0, Float z1, Float x, bool flip_normal = false);
	int Kind() const override { return JP_SHAPE_RECTANGLE; }
	FPoint3 p0, p1, p2, p3; FNormal3 normal;
};

class FSphere : public FShape                                    // shape.h:476-662
{
public:
	FSphere(const FVector3& center, Float r);
	int Kind() const override { return JP_SHAPE_SPHERE; }
	FVector3 center; Float radius;
};

class FDisk : public FShape                                      // shape.h:189-275
{
public:
	FDisk(const FPoint3& pos, const FVector3& normal, Float radius);
	int Kind() const override { return JP_SHAPE_DISK; }
	FPoint3 position; FVector3 normal; Float radius;             // normal normalised by the constructor (shape.h:194)
};

// triangulated OBJ ingest with the reference's transform order (shape.cc:23-68): z flip, scale, offset; `vt` texture coordinates ride along
// untransformed (faces v, v/vt, v/vt/vn, v//vn; negative indices count back; a face without vt gets uv 0).  `vn` normals are used only when `smoothing`
// asks for them: flip_normal negates them, bFlipHandedness mirrors them as it mirrors positions, offset and the uniform scale leave them alone.
bool LoadTriangleMesh(const char* filename, std::vector<std::shared_ptr<FTriangle>>& outTriangles, bool flip_normal = false,
                      bool bFlipHandedness = false, const FVector3& offset = FVector3(0, 0, 0), Float inScale = 1.f, const FSmoothing& smoothing = FSmoothing());

// ---- textures (texture.h / texture.cc): descriptions, sampled on the device (JpTextures) ------------------------
class FTexture
{
public:
	virtual ~FTexture() {}
	virtual int Kind() const = 0;                                // JP_TEXTURE_*
};
class FSolidColor : public FTexture                              // texture.h
{
public:
	FSolidColor() {}
	FSolidColor(const FColor& c) : color(c) {}
	FSolidColor(Float r, Float g, Float b) : color(r, g, b) {}
	int Kind() const override { return JP_TEXTURE_SOLID; }
	FColor color;
};
class FCheckerTexture : public FTexture                          // texture.h, texture.cc (Sample)
{
public:
	FCheckerTexture(const FColor& t0, const FColor& t1) : odd(t0), even(t1) {}
	int Kind() const override { return JP_TEXTURE_CHECKER; }
	FColor odd, even;
};
// ---- procedural textures (include/jetpbrt_amd.h "Procedural textures", include/jp_procedural.h): gradient noise, fBm, turbulence, marble and the box-filtered
// checker between two colours (even at t = 0, odd at t = 1, both in [0, 1]); flattened as a CHECKER texture plus its record (jp_set_texture_procedurals).
// transform: the row-major 3 x 4 map of the hit point (or of (u, v, 0) with uvSpace) into texture space, null: the identity; octaves 0: 6; gain 0: 0.5;
// antialias: band-limit by the footprint of the path's ray cone.
class FProceduralTexture : public FCheckerTexture
{
public:
	FProceduralTexture(int kind, const FColor& odd, const FColor& even, const float* transform, int octaves, Float gain, bool antialias, Float variation = 0, bool uvSpace = false)
		: FCheckerTexture(odd, even)
	{
		static const float identity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
		record.kind = kind; record.space = uvSpace ? JP_PROC_SPACE_UV : JP_PROC_SPACE_WORLD;
		for (int k = 0; k < 12; k++) record.m[k] = transform ? transform[k] : identity[k];
		record.octaves = octaves; record.gain = gain; record.variation = variation; record.antialias = antialias ? 1 : -1;
	}
	// every factory takes the colours in the constructor's (and FCheckerTexture's) order: odd (t = 1) first, then even (t = 0)
	static std::shared_ptr<FProceduralTexture> Noise(const FColor& odd, const FColor& even, const float* transform = nullptr, int octaves = 0, Float gain = 0, bool antialias = true)
	{ return std::make_shared<FProceduralTexture>(JP_PROC_NOISE, odd, even, transform, octaves, gain, antialias); }
	static std::shared_ptr<FProceduralTexture> FBm(const FColor& odd, const FColor& even, const float* transform = nullptr, int octaves = 0, Float gain = 0, bool antialias = true)
	{ return std::make_shared<FProceduralTexture>(JP_PROC_FBM, odd, even, transform, octaves, gain, antialias); }
	static std::shared_ptr<FProceduralTexture> Turbulence(const FColor& odd, const FColor& even, const float* transform = nullptr, int octaves = 0, Float gain = 0, bool antialias = true)
	{ return std::make_shared<FProceduralTexture>(JP_PROC_TURBULENCE, odd, even, transform, octaves, gain, antialias); }
	static std::shared_ptr<FProceduralTexture> Marble(const FColor& odd, const FColor& even, const float* transform = nullptr, int octaves = 0, Float gain = 0, bool antialias = true, Float variation = 0)
	{ return std::make_shared<FProceduralTexture>(JP_PROC_MARBLE, odd, even, transform, octaves, gain, antialias, variation); }
	static std::shared_ptr<FProceduralTexture> FilteredChecker(const FColor& odd, const FColor& even, const float* transform = nullptr, bool antialias = true)   // (a checker has no octaves)
	{ return std::make_shared<FProceduralTexture>(JP_PROC_CHECKER_AA, odd, even, transform, 0, 0, antialias); }
	JpProcedural record;
};
// ---- texture sampling (include/jetpbrt_amd.h "Texture sampling"): how an image texture or a normal map is addressed; the default is the identity record ----
enum class EWrap { Clamp = JP_WRAP_CLAMP, Repeat = JP_WRAP_REPEAT, Mirror = JP_WRAP_MIRROR };
enum class EFilter { Default = JP_FILTER_DEFAULT, Nearest = JP_FILTER_NEAREST, Bilinear = JP_FILTER_BILINEAR };   // Default: nearest for an image texture, bilinear for a normal map
struct FTexSampling
{
	EWrap wrapU = EWrap::Clamp, wrapV = EWrap::Clamp;
	EFilter filter = EFilter::Default;
	Float scaleU = 1, scaleV = 1, offsetU = 0, offsetV = 0;      // t = c * scale + offset per axis
	JpTexSampler Record() const { JpTexSampler r = { (int32_t)wrapU, (int32_t)wrapV, (int32_t)filter, scaleU, scaleV, offsetU, offsetV }; return r; }
};

class FImageTexture : public FTexture                            // texture.h, texture.cc (constructor, Sample)
{
public:
	const static int bytes_per_pixel = 3;
	FImageTexture() : width(0), height(0) {}
	// binary PPM (P6, maxval 255) or uncompressed 24 / 32-bit BMP (film_io.cc); anything else prints the reference's error and samples
	// as solid cyan (0, 1, 1), the reference's debugging aid
	FImageTexture(const char* filename);
	FImageTexture(const uint8_t* rgb8, int w, int h);           // RGB8, row-major, top row first
	int Kind() const override { return data.empty() ? JP_TEXTURE_SOLID : JP_TEXTURE_IMAGE; }
	std::vector<uint8_t> data;                                   // empty: no image (solid cyan)
	int width, height;
	// the texture's own sampling record (jp_set_texture_sampling); unset: the command line's defaults where given, else the identity
	void SetSampling(const FTexSampling& s) { sampling = s; hasSampling = true; }
	FTexSampling sampling; bool hasSampling = false;
	// mip maps (jp_set_texture_mipmaps): trilinear filtering at the footprint of the path's ray cone; unset: the scene's default (FScene::SetTextureMipmapDefault), else off
	void SetMipmaps(bool on) { mipmaps = on; hasMipmaps = true; }
	bool mipmaps = false, hasMipmaps = false;
};
// image readers of film_io.cc: RGB8, top row first; false for any other format or a file that cannot be read
bool ReadImageRGB8(const char* filename, std::vector<uint8_t>& rgb, int& width, int& height);

// ---- environment map (include/jetpbrt_amd.h "Environment maps"): a lat-long float image, top row first, the light of FScene::SetEnvironmentMap ----
// Float readers of film_io.cc; false (with a message) for a file that cannot be read, is malformed or truncated, holds a value that is negative or not
// finite, or is not 1 .. 4096 texels per side.  PFM: "PF" (colour) or "Pf" (grey, copied to the three channels), rows bottom first as the format has them,
// either byte order (the scale line's sign; its magnitude is not applied).  HDR: Radiance RGBE, "-Y h +X w", flat pixels as FFilm::SaveAsImage writes
// them or the run-length encoded scanlines other writers produce.
bool ReadImagePFM(const char* filename, std::vector<float>& rgb, int& width, int& height, std::string* error = nullptr);
bool ReadImageHDR(const char* filename, std::vector<float>& rgb, int& width, int& height, std::string* error = nullptr);
class FEnvironmentMap
{
public:
	FEnvironmentMap(const float* rgb, int w, int h);                // from memory: 3 * w * h floats, row-major, top row first
	// by content: PFM, Radiance .hdr, or binary PPM / uncompressed BMP through ReadImageRGB8 at 1/255 per step; null (with a message) when the file is refused
	static std::shared_ptr<FEnvironmentMap> FromFile(const char* filename, std::string* error = nullptr);
	bool Valid() const { return width > 0 && height > 0 && data.size() == (size_t)width * height * 3; }
	std::vector<float> data;
	int width = 0, height = 0;
	unsigned long long id;                                         // distinct per object: how an integrator tells which map its context holds
};

// ---- normal map (include/jetpbrt_amd.h "Normal maps"): an RGB8 tangent-space map, top row first, the FMaterial::normalMap of any material ----
class FNormalMap
{
public:
	FNormalMap(const uint8_t* rgb8, int w, int h);                  // from memory: 3 * w * h bytes, row-major, top row first
	// binary PPM or uncompressed BMP through ReadImageRGB8; null when the file is refused
	static std::shared_ptr<FNormalMap> FromFile(const char* filename);
	// a height map (w * h grey bytes, top row first) as a normal map: central differences with clamped neighbours, heights in 0 .. 1,
	// n = normalize(-scale * dh/dx, -scale * dh/dy_up, 1) per texel, each component encoded as round(127 * c) + 128 (the inverse of the decode)
	static std::shared_ptr<FNormalMap> FromHeight(const uint8_t* grey, int w, int h, float scale);
	// a w x h height image baked from a procedural record with the host lookup (include/jp_procedural.h; t over uv in [0, 1)^2 at z = 0, width 0: q = M (u, v, 0) + t,
	// whatever the record's space), then FromHeight: a marble floor can be bumpy too.  Null for a record the validation refuses or a size out of range.
	static std::shared_ptr<FNormalMap> FromProcedural(const JpProcedural& record, int w, int h, float scale);
	bool Valid() const { return width >= 1 && width <= 16384 && height >= 1 && height <= 16384 && data.size() == (size_t)width * height * 3; }
	std::vector<uint8_t> data;
	int width = 0, height = 0;
	// the map's sampling record (jp_set_texture_sampling): Clamp or Repeat, the bilinear filter, scales > 0
	void SetSampling(const FTexSampling& s) { sampling = s; hasSampling = true; }
	FTexSampling sampling; bool hasSampling = false;
};

// ---- materials: parameter holders with a flatten hook -------------------------------------------------------
class FMaterial
{
public:
	virtual ~FMaterial() {}
	virtual int Kind() const = 0;                                // JP_MAT_*
	virtual void Flatten(float out[JP_MAT_PARAM_STRIDE]) const = 0;
	// the texture of the main colour (matte, mirror, plastic); FlattenScene refuses one on glass or metal, whose [0..2] is eta
	std::shared_ptr<FTexture> texture;
	// a tangent-space normal map on any material kind (jp_set_normal_maps): the shading normal is perturbed by the map at the hit's uv, x and y scaled by normalStrength
	std::shared_ptr<FNormalMap> normalMap; Float normalStrength = 1;
};
Float RoughnessToAlpha(Float roughness);                         // microfacet.h:85-90

class FMatteMaterial : public FMaterial                          // material.h:27-41
{ public: FMatteMaterial(const FColor& c) : diffuseColor(c) {} FMatteMaterial(const std::shared_ptr<FTexture>& tex) { texture = tex; }
  int Kind() const override { return JP_MAT_MATTE; } void Flatten(float*) const override; FColor diffuseColor; };
class FMirrorMaterial : public FMaterial                         // material.h:45-59
{ public: FMirrorMaterial(const FColor& c) : specularColor(c) {} FMirrorMaterial(const std::shared_ptr<FTexture>& tex) { texture = tex; }
  int Kind() const override { return JP_MAT_MIRROR; } void Flatten(float*) const override; FColor specularColor; };
class FGlassMaterial : public FMaterial                          // material.h:63-81
{ public: FGlassMaterial(Float eta, const FColor& kr = FColor(1, 1, 1), const FColor& kt = FColor(1, 1, 1)) : eta(eta), Kr(kr), Kt(kt) {}
  int Kind() const override { return JP_MAT_GLASS; } void Flatten(float*) const override; Float eta; FColor Kr, Kt; };
class FPlasticMaterial : public FMaterial                        // material.h:85-110, material.cc:12-29
{ public: FPlasticMaterial(const FColor& Kd, const FColor& Ks, Float roughness, bool remapRoughness);
  // textured Kd: Qd follows the sampled Kd at every shading point (Ld = Kd.Luminance(), Qd = Ld / (Ld + Ks.Luminance()), on the device)
  FPlasticMaterial(const std::shared_ptr<FTexture>& tex, const FColor& Ks, Float roughness, bool remapRoughness);
  int Kind() const override { return JP_MAT_PLASTIC; } void Flatten(float*) const override; FColor Kd, Ks; Float roughness; bool remapRoughness; Float Qd; };
class FMetalMaterial : public FMaterial                          // material.h:113-137, material.cc:31-43
{ public: FMetalMaterial(const FColor& eta, const FColor& k, Float ur, Float vr, bool remap) : eta(eta), k(k), uRoughness(ur), vRoughness(vr), remapRoughness(remap) {}
  int Kind() const override { return JP_MAT_METAL; } void Flatten(float*) const override; FColor eta, k; Float uRoughness, vRoughness; bool remapRoughness; };

// ---- lights -------------------------------------------------------------------------------------------------
class FScene;
enum eLightFlags { DeltaPosition = 1, DeltaDirection = 2, AreaLight = 4, InfiniteLight = 8 };   // light.h:16-23

class FLight
{
public:
	virtual ~FLight() {}
	FLight(int flags) : lightFlags(flags) {}
	int Flags() const { return lightFlags; }
	virtual int Kind() const = 0;                                // JP_LIGHT_*
	virtual void Preprocess(const FScene&) {}
	int lightFlags;
};
class FAreaLight : public FLight                                 // light.h:183-244
{ public: FAreaLight(const FPoint3&, int, const FColor& radiance, const FShape* shape) : FLight(eLightFlags::AreaLight), radiance(radiance), shape(shape) {}
  int Kind() const override { return JP_LIGHT_AREA; } FColor radiance; const FShape* shape; };
class FEnvironmentLight : public FLight                          // light.h:248-311, light.cc:26-33
{ public: FEnvironmentLight(const FPoint3&, int, const FColor& radiance) : FLight(eLightFlags::InfiniteLight), radiance(radiance), worldRadius(0) {}
  int Kind() const override { return JP_LIGHT_ENVIRONMENT; } void Preprocess(const FScene& scene) override; FColor radiance; FPoint3 worldCenter; Float worldRadius; };

class FPointLight : public FLight                                // light.h:81-132
{ public: FPointLight(const FPoint3& worldpos, int, const FColor& intensity) : FLight(eLightFlags::DeltaPosition), worldPosition(worldpos), intensity(intensity) {}
  int Kind() const override { return JP_LIGHT_POINT; } FPoint3 worldPosition; FColor intensity; };
class FDirectionLight : public FLight                            // light.h:136-180, light.cc:17-24
{ public: FDirectionLight(const FPoint3&, int, const FColor& irradiance, const FVector3& worlddir) : FLight(eLightFlags::DeltaDirection), irradiance(irradiance), worldDir(Normalize(worlddir)), worldRadius(0) {}
  int Kind() const override { return JP_LIGHT_DIRECTION; } void Preprocess(const FScene& scene) override; FColor irradiance; FVector3 worldDir; FPoint3 worldCenter; Float worldRadius; };

struct FPrimitive                                                // primitive.h:20-64
{
	const FShape* shape; const FMaterial* material; const FAreaLight* arealight;
	FPrimitive(const FShape* s, const FMaterial* m, const FAreaLight* l) : shape(s), material(m), arealight(l) {}
};

// ---- sampler / camera / film ----------------------------------------------------------------------------------
struct FCameraSample { FPoint2 posfilm; };

class FSampler                                                   // sampler.h:64-105 (description only: the draws happen on the device)
{
public:
	virtual ~FSampler() {}
	FSampler(int spp) : samples_per_pixel(spp) {}
	virtual std::unique_ptr<FSampler> Clone() = 0;
	virtual int GetSamplesPerPixel() { return samples_per_pixel; }
	virtual void SetSamplesPerPixel(int s) { samples_per_pixel = s; }
	virtual uint32_t Seed() const = 0;
	virtual int Mode() const { return JP_SAMPLER_COUNTER; }     // JpRenderParams::sampler_mode
protected:
	int samples_per_pixel;
};
// The counter stream of include/jp_counter_rng.h.
class FCounterSampler : public FSampler
{ public: FCounterSampler(int spp, uint32_t seed = 1234) : FSampler(spp), seed(seed) {} std::unique_ptr<FSampler> Clone() override { return std::make_unique<FCounterSampler>(samples_per_pixel, seed); }
  uint32_t Seed() const override { return seed; } uint32_t seed; };
// Drop-in for main.cc:149.  The stock sequential mt19937_64 stream cannot be reproduced in parallel, so a
// "random sampler" is served by the counter stream with the stock seed 1234 (sampler.h:26): same
// distribution, different random numbers.
class FRandomSampler : public FCounterSampler { public: FRandomSampler(int spp) : FCounterSampler(spp, 1234) {} };
// sampler.h:160-185: the reference's stratified sampler is an unfinished copy of its random sampler ("TODO") -- the same here
class FStratifiedSampler : public FCounterSampler { public: FStratifiedSampler(int spp) : FCounterSampler(spp, 1234) {} };
// sampler.h:109-127: every draw is 0.5 and the camera sample is the pixel centre (the reference's GetCameraSample computes
// posfilm + (0.5, 0.5) but lacks its return statement); served by the device's JP_SAMPLER_DEBUG mode
class FDebugSampler : public FSampler
{ public: FDebugSampler(int spp) : FSampler(spp) {} std::unique_ptr<FSampler> Clone() override { return std::make_unique<FDebugSampler>(samples_per_pixel); }
  uint32_t Seed() const override { return 0; } int Mode() const override { return JP_SAMPLER_DEBUG; } };

class FCamera                                                    // camera.h:32-70
{
public:
	virtual ~FCamera() {}
	FCamera(const FVector3& ipos, const FVector3& ifront, const FVector3& iup, Float ifov, const FVector2& iresolution);
	FVector3 pos, front, right, up; FVector2 resolution;
	// Thin lens (INTEGRATION.md "Lens"; the reference's camera is the pinhole, radius 0): an aperture of `radius` scene units -- a disk (blades 0) or a regular polygon of
	// 3 .. 16 blades, its first vertex `rotation` degrees from `right` toward `up` -- focused on the plane pos + focus * d0 (depth focus * |front| along front).  Render-time
	// state: FGpuPathIntegrator::Render forwards it to jp_set_lens, no new upload.  FocusAt: the focus distance comes from jp_focus_distance at render time, after the
	// upload -- whatever the pinhole ray through film position (fx, fy) (pixels) hits is in focus; LastFocus() then tells the distance found (a miss fails the render).
	void SetLens(Float radius, Float focus, int blades = 0, Float rotation = 0) { lensRadius = radius; lensFocus = focus; lensBlades = blades; lensRotation = rotation; focusAt = false; }
	void FocusAt(Float fx, Float fy) { focusAt = true; focusFx = fx; focusFy = fy; }
	Float LastFocus() const { return lastFocus; }
	Float lensRadius = 0, lensFocus = 1, lensRotation = 0; int lensBlades = 0;
	bool focusAt = false; Float focusFx = 0, focusFy = 0;
	mutable Float lastFocus = 0;                                 // the focus distance of the last render with a lens
	// Projection (INTEGRATION.md "Projections"; the reference's camera is the perspective pinhole, JP_PROJ_PERSPECTIVE): JP_PROJ_ORTHOGRAPHIC (orthoScale: the width of
	// the view in units of |right|; 0: 1), JP_PROJ_EQUIRECT (a lat-long panorama around pos) or JP_PROJ_FISHEYE (equidistant; fovDeg in (0, 360], 0: 180, reached at the
	// half-diagonal, half-width or half-height: JP_FIT_*).  Render-time state like the lens: FGpuPathIntegrator::Render forwards it to jp_set_projection, no new upload.
	// CheckProjection: the library's own validation (jp_check_projection, no GPU needed) -- true, or false with its message.
	void SetProjection(int kind, Float orthoScale = 0, Float fovDeg = 0, int fit = JP_FIT_DIAGONAL) { projKind = kind; projOrthoScale = orthoScale; projFovDeg = fovDeg; projFit = fit; }
	bool CheckProjection(std::string* message = nullptr) const;
	int projKind = JP_PROJ_PERSPECTIVE, projFit = JP_FIT_DIAGONAL; Float projOrthoScale = 0, projFovDeg = 0;
};

enum class EImageType { PPM, BMP, HDR };                         // film.h:15-20

inline Float Clamp01(Float x) { return x < 0 ? 0 : (x > 1 ? 1 : x); }                                   // film.h:22
inline uint8_t gamma_encoding(Float x) { return (uint8_t)(std::pow(Clamp01(x), (Float)(1 / 2.2)) * 255.0); }   // film.h:24

// FFilm::RequestDenoise: the fields of JpDenoiseParams (0: the library's default; INTEGRATION.md "Guides and denoising")
// varianceGuided: the variance-guided filter (jp_denoise_variance; INTEGRATION.md "Variance") on a variance render instead of jp_denoise on a plain one
struct FDenoiseOptions { int iterations = 0; Float sigmaColor = 0, sigmaNormal = 0, sigmaDepth = 0; bool demodulate = true; bool varianceGuided = false; };
// FFilm::SetToneMap: the fields of JpToneMap (curve: JP_CURVE_*; 0: the library's default; INTEGRATION.md "Film")
struct FToneMap { int curve = JP_CURVE_CLAMP; bool autoExposure = false; Float ev = 0, key = 0, white = 0, pctLow = 0, pctHigh = 0; };

class FFilm                                                      // film.h:27-94
{
public:
	FFilm(int w, int h) : width(w), height(h), pixels((size_t)w * h) {}
	int Width() const { return width; } int Height() const { return height; }
	FVector2 GetResolution() const { return FVector2((Float)width, (Float)height); }
	// (writable access: the 8-bit bytes the device delivered describe the film as it was rendered, so any change drops them)
	FColor& operator()(int x, int y) { InvalidateLDR(); return pixels[(size_t)width * y + x]; }
	const FColor& operator()(int x, int y) const { return pixels[(size_t)width * y + x]; }
	void AddColor(int x, int y, const FColor& c) { FColor& p = (*this)(x, y); p.r += c.r; p.g += c.g; p.b += c.b; }
	void Clear() { InvalidateLDR(); for (auto& p : pixels) p = FColor(); }
	void InvalidateLDR() { if (!ldr8.empty()) { ldr8.clear(); floatValid = true; } }
	// the output step right after the hot path (main.cc:160): <filename>.ppm/.bmp/.hdr, gamma 1/2.2 for the 8-bit formats
	bool SaveAsImage(const std::string& filename, EImageType imgType) const;
	// Tone mapping on the GPU: ask the integrator for the film as 8-bit gamma-encoded RGB (gamma_encoding of film.h:24 applied on
	// the device after the resolve, byte-identical to the host's) next to -- or, with ldrOnly, INSTEAD of -- the fp32 pixels: a
	// BMP / PPM then costs a 3-bytes-per-pixel download instead of 12.  SaveAsImage writes ldr8 when it is present.
	void RequestDeviceLDR(bool only = true) { wantLDR = true; ldrOnly = only; }
	bool HasLDR() const { return ldr8.size() == (size_t)width * height * 3; }
	// Guides and denoising: ask the integrator for the first-hit feature buffers of the frame (guideSpp camera samples per pixel) and, with
	// RequestDenoise, for the edge-avoiding filter they steer: after Render the film holds the DENOISED image (added onto the film like every
	// render result; with RequestDeviceLDR the bytes are its tone map) and Albedo() / Normal() / Depth() hold the guides, row-major, top row first.
	void RequestDenoise(int guideSpp = 8, const FDenoiseOptions& options = FDenoiseOptions()) { wantGuides = wantDenoise = true; guideSpp_ = guideSpp; denoise = options; }
	void RequestGuides(int guideSpp = 8) { wantGuides = true; guideSpp_ = guideSpp; }
	const std::vector<FColor>& Albedo() const { return albedo; }
	const std::vector<FVector3>& Normal() const { return normal; }
	const std::vector<Float>& Depth() const { return depth; }
	// Variance (INTEGRATION.md "Variance"): ask the integrator for the per-pixel variance of the film's mean luminance (jp_render_variance; needs spp >= 2): after
	// Render Variance() holds the plane, row-major, top row first; the film is the one a plain Render delivers.  Together with RequestDenoise it needs the
	// variance-guided filter (FDenoiseOptions::varianceGuided), which reads that plane; that filter asks for the variance render by itself.
	void RequestVariance() { wantVariance = true; }
	const std::vector<Float>& Variance() const { return variance; }
	// Adaptive sampling (INTEGRATION.md "Adaptive sampling"): the integrator stops each pixel once the relative standard error of its mean luminance is below
	// `threshold` (jp_render_adaptive: minSpp samples everywhere, then stepSpp more per pass for the pixels still above it -- with dilate, and their neighbours -- up
	// to the sampler's samples per pixel).  After Render SampleCounts() holds the samples each pixel took and Variance() the variance of its mean, row-major, top
	// row first; with RequestDenoise(n, { varianceGuided }) the filter reads that plane.  The path integrator only; not together with a device tone map or LDR film.
	void SetAdaptive(Float threshold, int minSpp = 8, int stepSpp = 8, bool dilate = true) { wantAdaptive = true; adaptThreshold = threshold; adaptMin = minSpp; adaptStep = stepSpp; adaptDilate = dilate; }
	const std::vector<int32_t>& SampleCounts() const { return sampleCounts; }
	// The linear-light film (INTEGRATION.md "Film"): SetHDR keeps radiance above 1 (SaveAsImage(HDR) then writes the unclamped film, and a denoise request filters
	// it unclamped), SetSampleClamp tames fireflies sample by sample, SetToneMap -- which turns HDR on: highlights above 1 are what the curves compress -- has the
	// integrator deliver the 8-bit bytes of BMP / PPM through exposure and a tone curve on the GPU (next to the fp32 film, or instead of it with RequestDeviceLDR).
	// ToneMapScale(): the exposure scale the last render's transform used (auto-exposure: from the film's luminance histogram).
	void SetHDR(bool on = true) { hdr = on; }
	void SetSampleClamp(Float c) { sampleClamp = c; }
	void SetToneMap(const FToneMap& t) { toneMap = t; haveToneMap = true; hdr = true; }
	Float ToneMapScale() const { return toneMapScale; }
	bool hdr = false, haveToneMap = false; Float sampleClamp = 0, toneMapScale = 0; FToneMap toneMap;
	bool wantGuides = false, wantDenoise = false; int guideSpp_ = 8; FDenoiseOptions denoise;
	std::vector<FColor> albedo; std::vector<FVector3> normal; std::vector<Float> depth;
	bool wantVariance = false; std::vector<Float> variance;
	bool wantAdaptive = false, adaptDilate = true; Float adaptThreshold = 0; int adaptMin = 8, adaptStep = 8; std::vector<int32_t> sampleCounts;
	int width, height; std::vector<FColor> pixels;
	bool wantLDR = false, ldrOnly = false; std::vector<uint8_t> ldr8;   // R G B per pixel, top row first
	bool floatValid = true;                                            // false after an LDR-only render: the fp32 pixels were not downloaded
};

// ---- reflection API (bsdf.h, bsdf.cc, microfacet.h, microfacet.cc) --------------------------------------------------------
// The reference's BSDF classes by name, for code that builds or probes a BSDF directly (the render path builds its closures on the
// device from the material table).  Objects only hold their parameters; Evalf / Pdf / Sample run ON THE DEVICE through jp_bsdf
// (k_bsdf, csrc/jp_xbsdf.h) -- there is no host implementation.  World-space vectors, frame = FFrame(normal) as in bsdf.h:284-302.
struct FFrame { FVector3 n; FFrame(const FVector3& nn) : n(nn) {} };                     // geometry.h:326-378 (built on the device)
struct FBSDFSample { FColor f; FVector3 wi; Float pdf = 0; int ebsdf = 0; };             // bsdf.h:252-265
class Fresnel { public: virtual ~Fresnel() {} virtual void Fill(JpBsdfDesc& d) const = 0; };               // bsdf.h:637-643
class FresnelConductor : public Fresnel                                                   // bsdf.h:645-655
{ public: FresnelConductor(const FColor& etaI, const FColor& etaT, const FColor& k) : etaI(etaI), etaT(etaT), k(k) {}
  void Fill(JpBsdfDesc& d) const override { d.fresnel = JP_FRESNEL_CONDUCTOR; d.fr_eta_i[0] = etaI.r; d.fr_eta_i[1] = etaI.g; d.fr_eta_i[2] = etaI.b; d.fr_eta_t[0] = etaT.r; d.fr_eta_t[1] = etaT.g; d.fr_eta_t[2] = etaT.b; d.fr_k[0] = k.r; d.fr_k[1] = k.g; d.fr_k[2] = k.b; }
  FColor etaI, etaT, k; };
class FresnelDielectric : public Fresnel                                                  // bsdf.h:657-662
{ public: FresnelDielectric(Float etaI, Float etaT) : etaI(etaI), etaT(etaT) {}
  void Fill(JpBsdfDesc& d) const override { d.fresnel = JP_FRESNEL_DIELECTRIC; d.fr_eta_i[0] = d.fr_eta_i[1] = d.fr_eta_i[2] = etaI; d.fr_eta_t[0] = d.fr_eta_t[1] = d.fr_eta_t[2] = etaT; }
  Float etaI, etaT; };
class FresnelNoOp : public Fresnel { public: void Fill(JpBsdfDesc& d) const override { d.fresnel = JP_FRESNEL_NOOP; } };   // bsdf.h:664-667
class MicrofacetDistribution                                                              // microfacet.h:16-39
{ public: virtual ~MicrofacetDistribution() {} MicrofacetDistribution(int kind, Float ax, Float ay, bool vis) : kind(kind), alphax(ax), alphay(ay), sampleVisibleArea(vis) {}
  int kind; Float alphax, alphay; bool sampleVisibleArea; };
class BeckmannDistribution : public MicrofacetDistribution                               // microfacet.h:42-63
{ public: BeckmannDistribution(Float ax, Float ay, bool samplevis = true) : MicrofacetDistribution(JP_DIST_BECKMANN, ax, ay, samplevis) {}
  static Float RoughnessToAlpha(Float roughness) { roughness = roughness < (Float)1e-3 ? (Float)1e-3 : roughness; Float x = std::log(roughness); return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x; } };
class TrowbridgeReitzDistribution : public MicrofacetDistribution                         // microfacet.h:65-99
{ public: TrowbridgeReitzDistribution(Float ax, Float ay, bool samplevis = true) : MicrofacetDistribution(JP_DIST_TROWBRIDGE_REITZ, ax, ay, samplevis) {}
  static Float RoughnessToAlpha(Float roughness) { return BeckmannDistribution::RoughnessToAlpha(roughness); } };
class FBSDF                                                                               // bsdf.h:268-332
{
public:
	virtual ~FBSDF() {}
	FBSDF(const FFrame& frame, int kind) : normal(frame.n) { desc = JpBsdfDesc(); desc.kind = kind; desc.color[0] = desc.color[1] = desc.color[2] = 1; desc.eta_a = 1; desc.eta_b = 1; desc.sample_visible = 1; }
	virtual bool IsDelta() const { return desc.kind == JP_BSDF_MIRROR || desc.kind == JP_BSDF_FRESNEL_SPECULAR; }
	FColor Evalf(const FVector3& world_wo, const FVector3& world_wi) const;
	Float Pdf(const FVector3& world_wo, const FVector3& world_wi) const;
	FBSDFSample Sample(const FVector3& world_wo, const FVector2& random) const;
	JpBsdfDesc desc; FVector3 normal;
protected:
	void SetColor(const FColor& c) { desc.color[0] = c.r; desc.color[1] = c.g; desc.color[2] = c.b; }
	void SetDist(const MicrofacetDistribution* d) { desc.distribution = d->kind; desc.alpha_x = d->alphax; desc.alpha_y = d->alphay; desc.sample_visible = d->sampleVisibleArea ? 1 : 0; }
};
class FLambertionReflection : public FBSDF { public: FLambertionReflection(const FFrame& f, const FColor& albedo) : FBSDF(f, JP_BSDF_LAMBERT) { SetColor(albedo); } };   // bsdf.h:336-385
class FSpecularReflection : public FBSDF { public: FSpecularReflection(const FFrame& f, const FColor& R) : FBSDF(f, JP_BSDF_MIRROR) { SetColor(R); } };                 // bsdf.h:394-435
class FFresnelSpecular : public FBSDF                                                     // bsdf.h:455-552
{ public: FFresnelSpecular(const FFrame& f, Float eta_i, Float eta_t, const FColor& Kr, const FColor& Kt) : FBSDF(f, JP_BSDF_FRESNEL_SPECULAR) { SetColor(Kr); desc.color2[0] = Kt.r; desc.color2[1] = Kt.g; desc.color2[2] = Kt.b; desc.eta_a = eta_i; desc.eta_b = eta_t; } };
class FPhongSpecularReflection : public FBSDF                                             // bsdf.h:557-633
{ public: FPhongSpecularReflection(const FFrame& f, const FColor& Ks, Float exponent) : FBSDF(f, JP_BSDF_PHONG) { SetColor(Ks); desc.exponent = exponent; } };
class FMicrofacetReflection : public FBSDF                                                // bsdf.h:676-701, bsdf.cc:29-78 (owns both objects, as the reference does)
{ public: FMicrofacetReflection(const FFrame& f, const FColor& R, MicrofacetDistribution* distribution, Fresnel* fresnel) : FBSDF(f, JP_BSDF_MICROFACET_REFLECTION), distribution(distribution), fresnel(fresnel) { SetColor(R); SetDist(distribution); fresnel->Fill(desc); }
  ~FMicrofacetReflection() { delete distribution; delete fresnel; }
  const MicrofacetDistribution* distribution; const Fresnel* fresnel; };
class FMicrofacetTransmission : public FBSDF                                              // bsdf.h:703-734, bsdf.cc:80-145
{ public: FMicrofacetTransmission(const FFrame& f, const FColor& T, MicrofacetDistribution* distribution, Float etaA, Float etaB) : FBSDF(f, JP_BSDF_MICROFACET_TRANSMISSION), distribution(distribution) { SetColor(T); SetDist(distribution); desc.eta_a = etaA; desc.eta_b = etaB; }
  ~FMicrofacetTransmission() { delete distribution; }
  const MicrofacetDistribution* distribution; };

// ---- scene ----------------------------------------------------------------------------------------------------
struct FlatBVH { std::vector<float> bounds; std::vector<int32_t> left, right, prim_index; };

class FScene                                                     // scene.h:23-150, scene.cc
{
public:
	FScene(const char* inName) : name(inName) {}
	const char* NameStr() const { return name.c_str(); }
	void Preprocess();                                           // world bound -> light preprocess -> BVH build (scene.cc:11-23)
	FBounds3 WorldBound() const { return worldBound; }
	const FCamera* Camera() const { return camera.get(); }
	int LightNum() const { return (int)lights.size(); }

	template<typename T, typename... U> std::shared_ptr<T> CreateCamera(const U&... args) { auto c = std::make_shared<T>(args...); camera = c; return c; }
	template<typename T, typename... U> std::shared_ptr<T> CreateShape(const U&... args) { auto s = std::make_shared<T>(args...); shapes.push_back(s); return s; }
	template<typename T, typename... U> std::shared_ptr<T> CreateMaterial(const U&... args) { auto m = std::make_shared<T>(args...); materials.push_back(m); return m; }
	template<typename T, typename... U> std::shared_ptr<T> CreateLight(const U&... args) { auto l = std::make_shared<T>(args...); lights.push_back(l); return l; }
	template<typename... U> std::shared_ptr<FPrimitive> CreatePrimitive(const U&... args) { auto p = std::make_shared<FPrimitive>(args...); primitives.push_back(p); return p; }

	std::vector<std::shared_ptr<FShape>> CreateTriangleMesh(const char* filename, bool flip_normal = false, bool bFlipHandedness = false, const FVector3& offset = FVector3(0, 0, 0), Float inScale = 1.f,
	                                                        const FSmoothing& smoothing = FSmoothing());
	std::vector<std::shared_ptr<FPrimitive>> CreatePrimitives(const std::vector<std::shared_ptr<FShape>>& inMesh, const std::shared_ptr<FMaterial>& inMaterial);
	std::vector<std::shared_ptr<FAreaLight>> CreateAreaLights(int samplesNum, const FColor& radiance, const std::vector<std::shared_ptr<FShape>>& inShapes, const std::shared_ptr<FMaterial>& inMaterial);
	std::shared_ptr<FAreaLight> CreateAreaLight(int samplesNum, const FColor& radiance, const std::shared_ptr<FShape>& inShape, const std::shared_ptr<FMaterial>& inMaterial);

	std::string name;
	std::shared_ptr<FCamera> camera;
	std::vector<std::shared_ptr<FShape>> shapes;
	std::vector<std::shared_ptr<FMaterial>> materials;
	std::vector<std::shared_ptr<FLight>> lights;
	std::vector<std::shared_ptr<FPrimitive>> primitives;
	FBounds3 worldBound;
	FlatBVH bvh;                                                 // built by Preprocess() unless deviceBuild
	bool preprocessed = false;
	// true: Preprocess() skips the host SAH build and the flattened scene carries no hierarchy (n_bvh_nodes = 0), so
	// jp_upload_scene builds the tree on the device (round 3: PLOC clustering, jp_ploc.h -- as fast to walk as the host's binned-SAH
	// tree on the 280k-triangle scene, setup 0.2 s -> 0.06 s; rounds 1-2: an LBVH, 7-18 % slower to walk).
	// Default (round 3): scenes of more than kDeviceBuildFrom primitives build on the device, smaller ones on the host (their trees
	// become flat leaf lists / LDS-resident trees, which need the host's leaves).  hostBuild = true or env JETPBRT_DEVICE_BVH=0 keep the
	// host build for every scene, deviceBuild = true or JETPBRT_DEVICE_BVH=1 force the device build.
	bool deviceBuild = false, hostBuild = false;
	bool builtOnDevice = false;                                  // what the last Preprocess() decided (read-only for callers)
	static constexpr size_t kDeviceBuildFrom = 4096;
	// true: Preprocess() builds the reference's own tree (BuildReferenceBVH: its rand() sequence from the default seed, its
	// std::sort, median split, leaves <= 5, over the reference's WorldBounds) and the flattened scene asks the device to walk
	// it with the reference's semantics (JpScene.bvh_reference_semantics): the film then equals the reference's bit for bit on
	// tessellated meshes too, at several times the traversal cost.  Default from env JETPBRT_REFERENCE_TREE=1.
	bool referenceTree = false;
	// With referenceTree: the CERTIFIED walk (JpScene.bvh_reference_semantics = 2; DESIGN.md "Certified walk") -- an ordered walk over the leaves
	// of the reference's tree that proves, ray by ray, that FBVH_Node::Intersect returns the same hit, and repeats the few rays it cannot prove
	// the reference's way.  About twice as fast as the verbatim walk on large meshes.  Outside the proof: a ray that lies within fp32 noise of a
	// triangle's plane is decided in the reference by the signs of rounding errors wherever that triangle is; camera rays are covered by flags on the
	// leaves edge-on to the camera, secondary rays only by measurement (the 280k-triangle frame is bit-identical).  Default from env JETPBRT_REFERENCE_TREE=2.
	bool certifiedWalk = false;
	// Light selection of the path integrator (include/jetpbrt_amd.h, INTEGRATION.md "Light selection"): JP_LIGHTS_ALL samples every light at every
	// bounce, the reference's estimator (at most 255 lights); JP_LIGHTS_POWER_ONE picks one light per bounce with probability proportional to its
	// power -- what a scene lit by CreateAreaLights(mesh) needs.  Read by FGpuPathIntegrator::Render at its next upload of this scene.
	int lightSampling = JP_LIGHTS_ALL;
	void SetLightSampling(int mode) { lightSampling = mode; }
	// The sampling record of every FImageTexture without one of its own (FImageTexture::SetSampling); unset: the identity.  Read by FlattenScene.
	FTexSampling textureSamplingDefault; bool hasTextureSamplingDefault = false;
	void SetTextureSamplingDefault(const FTexSampling& s) { textureSamplingDefault = s; hasTextureSamplingDefault = true; }
	// Mip maps of every FImageTexture without a choice of its own (FImageTexture::SetMipmaps); the footprint's scale (0: 1) and the least spread of the ray cone after a bounce
	// that is not specular (radians; 0: 0.125, a design choice) hold for the whole scene.  Read by FlattenScene.
	bool textureMipmapDefault = false; Float mipFootprintScale = 0, mipBounceSpread = 0;
	void SetTextureMipmapDefault(bool on = true) { textureMipmapDefault = on; }
	// JP_ESTIMATOR_NEE (default: the reference's estimator) or JP_ESTIMATOR_MIS: next-event estimation and the BSDF sample weighted against each other (power
	// heuristic).  Render-time state, sent before every render; a scene that asks for MIS is uploaded with JP_LIGHTS_POWER_ONE whatever lightSampling says.
	int estimator = JP_ESTIMATOR_NEE;
	void SetEstimator(int mode) { estimator = mode; }
	// Image-based lighting (INTEGRATION.md "Environment maps"): the scene's one FEnvironmentLight takes its radiance from `map` (the light's own
	// radiance tints it), looked up by nearest texel on a miss and importance-sampled by texel; up_axis JP_ENV_UP_Z / JP_ENV_UP_Y.  A mapped scene
	// renders with JP_LIGHTS_POWER_ONE whatever lightSampling says; one with no FEnvironmentLight, or more than one, is refused by Render.
	// nullptr: no map.  Read by FGpuPathIntegrator::Render at its next upload of this scene.
	std::shared_ptr<FEnvironmentMap> environmentMap; int environmentUp = JP_ENV_UP_Z, environmentImportance = 0;
	void SetEnvironmentMap(const std::shared_ptr<FEnvironmentMap>& map, int up_axis = JP_ENV_UP_Z) { environmentMap = map; environmentUp = up_axis; }
};

// binned-SAH BVH over primitive bounds -> the flat node arrays of JpScene (own topology)
void BuildBVH(const std::vector<FBounds3>& primBounds, FlatBVH& out, int maxLeaf = 4);
// the reference's tree node for node (bvh.h:54-146 with glibc's rand() from seed 1), over the reference's WorldBounds
void BuildReferenceBVH(const std::vector<FBounds3>& primWorldBounds, FlatBVH& out);

// the flattener: owns the SoA storage a JpScene view points into
struct FlatScene
{
	JpScene view;
	std::vector<float> tri_p0, tri_p1, tri_p2, tri_n, rect_p0, rect_p1, rect_p2, rect_p3, rect_n, sph_center, sph_radius;
	std::vector<float> disk_center, disk_normal, disk_radius;
	std::vector<int32_t> prim_shape_type, prim_shape_index, prim_material, prim_light, mat_type, light_type, light_prim;
	std::vector<float> mat_params, light_radiance, light_vec;
	FlatBVH bvh;
	// textures (jp_upload_scene_textured): filled only for a scene with a textured material (textures.n_textures == 0 otherwise);
	// shared textures are flattened once (by pointer)
	JpTextures textures;
	std::vector<int32_t> tex_type, tex_width, tex_height, mat_texture;
	std::vector<float> tex_color, tri_uv;
	std::vector<int64_t> tex_offset;
	std::vector<uint8_t> texels;
	// vertex normals (jp_set_vertex_normals): nine floats per triangle in tri_* order, nine zeros for a flat one; n_smooth == 0: the scene has none
	JpVertexNormals normals;
	std::vector<float> tri_vn; int n_smooth = 0;
	// normal maps (jp_set_normal_maps): shared maps are flattened once (by pointer); tri_uv is the textures'; n_normal_mapped == 0: the scene has none
	JpNormalMaps normalMaps;
	std::vector<int32_t> nm_width, nm_height, mat_normal_map; std::vector<int64_t> nm_offset; std::vector<uint8_t> nm_texels; std::vector<float> mat_normal_strength;
	int n_normal_mapped = 0;
	// texture sampling (jp_set_texture_sampling): one record per flattened texture and per flattened map, in their order; n_sampled == 0: every record is
	// the identity and the scene sets no sampling state
	JpTextureSampling sampling;
	std::vector<JpTexSampler> tex_sampler, nm_sampler;
	int n_sampled = 0;
	// mip maps (jp_set_texture_mipmaps): one mode per flattened texture; n_mipmapped == 0: every mode is OFF and the scene sets no mipmap state
	JpTextureMipmaps mipmaps;
	std::vector<int32_t> tex_mip_mode;
	int n_mipmapped = 0;
	// procedural textures (jp_set_texture_procedurals): one record per flattened texture; n_procedural == 0: every kind is NONE and the scene sets no such state
	JpTextureProcedurals procedurals;
	std::vector<JpProcedural> tex_procedural;
	int n_procedural = 0;
};
bool FlattenScene(const FScene& scene, FlatScene& out, std::string* error = nullptr);

// ---- integrator -------------------------------------------------------------------------------------------------
class FIntegrator
{
public:
	virtual ~FIntegrator() {}
	// same contract as integrator.h:32 / integrator.cc:35-80: blocking, results ADDED onto `film` (film.h:64-68)
	virtual void Render(const FScene* scene, FSampler* sampler, FFilm* film, int numthreads = 1) const = 0;
};

// FPathIntegratorIteration (integrator.h:109-122, integrator.cc:316-403) executed by the HIP wavefront kernels.
// `numthreads` is accepted for signature compatibility and ignored.  Failures (no GPU, library missing, bad
// scene) print through PBRT-style stderr logging and leave the film untouched -- the reference's error
// convention; there is NO CPU fallback.  LastStatus() exposes the JpStatus.
class FGpuPathIntegrator : public FIntegrator
{
public:
	explicit FGpuPathIntegrator(int maxDepth, int deviceId = 0);
	~FGpuPathIntegrator();
	void Render(const FScene* scene, FSampler* sampler, FFilm* film, int numthreads = 1) const override;
	int LastStatus() const { return lastStatus; }
	const JpCounters& Counters() const { return counters; }
	// multi-GPU band sharding (JpRenderParams::shard_*); default renders the whole film
	void SetShard(int index, int count, int bandRows = 20) { shardIndex = index; shardCount = count; this->bandRows = bandRows; }
	// ABI 7: the library's switches by value (JpOptions of include/jetpbrt_amd.h: stream lanes, traversal overrides, certified-walk slack, ...);
	// zero-initialised = the defaults.  Handed to jp_set_options before the next upload / render.
	void SetOptions(const JpOptions& o) { options = o; options.struct_bytes = (int32_t)sizeof(JpOptions); optionsDirty = true; uploaded = nullptr; }
	const JpOptions& Options() const { return options; }
protected:
	JpOptions options = {};
	mutable bool optionsDirty = false;
	int maxDepth, deviceId;
	int shardIndex = 0, shardCount = 1, bandRows = 20;
	mutable JpContext* ctx = nullptr;
	mutable const FScene* uploaded = nullptr;
	mutable int ctxEstimator = JP_ESTIMATOR_NEE;                    // the estimator the context was last told (FScene::SetEstimator)
	mutable int uploadedLights = JP_LIGHTS_ALL, ctxLights = JP_LIGHTS_ALL;   // FScene::lightSampling of the uploaded scene; the mode the context was last told
	mutable unsigned long long uploadedEnv = 0, ctxEnv = 0; mutable int uploadedEnvUp = 0, ctxEnvUp = 0, uploadedEnvImp = 0, ctxEnvImp = 0;   // FEnvironmentMap::id (0: none), up axis and importance: of the uploaded scene; last sent to the context
	mutable JpProjection ctxProjection = {};                        // the projection the context was last told (FCamera::SetProjection; kind 0: none)
	mutable JpLens ctxLens = {};                                    // the lens the context was last told (FCamera::SetLens; radius 0: none)
	mutable JpFilm ctxFilm = {}; mutable JpToneMap ctxToneMap = {};   // the film state and tone map the context was last told (FFilm::SetHDR / SetSampleClamp / SetToneMap; zeros: none)
	mutable bool ctxNormalMaps = false;                            // ... or normal maps (jp_set_normal_maps)
	mutable bool ctxProcedurals = false;                           // ... or procedural records (jp_set_texture_procedurals)
	mutable bool ctxMipmaps = false;                               // ... or mipmap modes (jp_set_texture_mipmaps)
	mutable bool ctxSampling = false;                              // ... or texture sampling records (jp_set_texture_sampling)
	mutable bool ctxNormals = false;                                // the context holds vertex normals of an earlier upload (jp_set_vertex_normals)
	mutable int lastStatus = 0;
	mutable JpCounters counters;
protected:
	int kind = JP_INTEGRATOR_PATH;                               // JpRenderParams::integrator
};
// the reference's other integrators behind the same Render() (integrator.h:44-85): device megakernel k_other, not the hot path
class FWhittedIntegrator : public FGpuPathIntegrator
{ public: explicit FWhittedIntegrator(int maxDepth, int deviceId = 0) : FGpuPathIntegrator(maxDepth, deviceId) { kind = JP_INTEGRATOR_WHITTED; } };
class FDebugIntegrator : public FGpuPathIntegrator
{ public: explicit FDebugIntegrator(int deviceId = 0) : FGpuPathIntegrator(0, deviceId) { kind = JP_INTEGRATOR_DEBUG_NORMAL; } };
typedef FGpuPathIntegrator FPathIntegratorIteration;             // main.cc:154 compiles unchanged
// FPathIntegratorRecursive (integrator.h:88-106, integrator.cc:233-307) is the same estimator written recursively: the same
// draws in the same order, emission on bounce 0 / after a specular bounce, NEE over all lights, roulette from bounce 3.  It
// differs from the iterative form only in how the throughput products are rounded (nested f * cos * Li / pdf instead of a
// running beta), i.e. in the last bits of a path's radiance -- measured against the reference's recursive integrator on the
// golden scenes: mean per-pixel L2 ~1e-8 (tests/test_gpu_parity.py).  The device serves it with the same kernels.
typedef FGpuPathIntegrator FPathIntegratorRecursive;

} // namespace jetpbrt
