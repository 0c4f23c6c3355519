// jet-pbrt_amd/host/cli_main.cc -- the reference's command line (main.cc:113-163) on the GPU integrator:
//     jetpbrt sceneid spp [width height] [--assets DIR] [--out NAME] [--format bmp|ppm|hdr] [--device-bvh | --reference-tree | --reference-tree=certified] [--integrator path|recursive|whitted|debug]
//             [--adaptive THRESHOLD [--min-spp N] [--spp-step N] [--no-adaptive-dilate]] [--denoise [variance]] [--guide-spp N] [--aov PREFIX] [--light-sampling all|power] [--estimator nee|mis] [--envmap FILE [--envmap-up y|z] [--envmap-scale S]] [--smooth file|DEG]
//             [--aperture R [--focus D | --focus-pixel X Y] [--blades N] [--aperture-rotation DEG]]
//             [--projection ortho|equirect|fisheye [--ortho-scale S] [--fisheye-fov DEG] [--fisheye-fit diagonal|width|height]]
//             [--normal-map FILE [--normal-strength S] [--normal-from-height SCALE]]
//             [--hdr] [--sample-clamp C] [--tonemap clamp|reinhard|aces|hable] [--exposure EV|auto] [--white W]
//             [--texture-wrap clamp|repeat|mirror] [--texture-filter nearest|bilinear] [--texture-tile SU SV] [--normal-wrap clamp|repeat] [--normal-tile SU SV]
//             [--texture-mip [--mip-footprint S] [--mip-bounce-spread RAD]]
//             [--floor-texture noise|fbm|turbulence|marble|checker [--floor-texture-scale S] [--floor-texture-octaves N] [--no-texture-antialias]]
// --floor-texture KIND: a procedural texture (FProceduralTexture) in world space on the floor of either scene, which gets a material of its own as with --normal-map;
// --floor-texture-scale S: texture-space units per world unit (default 0.02: one noise cell is 50 units wide); --floor-texture-octaves N: 1 .. 12 (default 6);
// --no-texture-antialias: point-sample it instead of band-limiting it by the footprint of the path's ray cone.
// --texture-mip: mip maps for every image texture (FScene::SetTextureMipmapDefault): trilinear filtering at the footprint of the path's ray cone; --mip-footprint S scales
// the footprint (default 1); --mip-bounce-spread RAD: the least spread of the cone after a bounce that is not specular (default 0.125, a design choice).
// --texture-wrap / --texture-filter / --texture-tile: the sampling record (FScene::SetTextureSamplingDefault) of every image texture without one of its own: the wrap mode of
// both axes, the filter, the uv scale; --normal-wrap / --normal-tile: the same for the --normal-map map (FNormalMap::SetSampling; a normal map is always filtered bilinearly).
// --hdr: the unclamped film (FFilm::SetHDR): --format hdr then writes radiance above 1.  --sample-clamp C: each sample's radiance is scaled down to a maximum channel of C
// before it enters the pixel's sum (FFilm::SetSampleClamp): fireflies.  --tonemap: the display transform of BMP / PPM on the GPU (FFilm::SetToneMap; implies --hdr):
// exposure, the curve, then the gamma table; --exposure EV: the scale 2^EV (default 0), auto: from the film's luminance histogram (key 0.18); --white W: Reinhard's
// white point (default 4).  The exposure scale used is echoed.
// --normal-map FILE: a tangent-space normal map (binary PPM or BMP; FMaterial::normalMap) on the floor of either scene -- the bunny scene's floor rectangle, the Cornell box's
// floor mesh, which then gets a material of its own and must carry `vt`; --normal-strength S scales the map's x and y (default 1); --normal-from-height SCALE reads FILE as a
// height map (its red channel) and derives the normals from it (FNormalMap::FromHeight).
// --aperture R: a thin lens of radius R scene units instead of the pinhole (FCamera::SetLens): depth of field.  --focus D: the focus distance (the plane of focus lies D * |front|
// along the viewing direction; default 1); --focus-pixel X Y: focus on whatever film position (X, Y) sees (FCamera::FocusAt; the distance found is echoed); --blades N: a regular
// polygon of 3 .. 16 blades instead of a disk; --aperture-rotation DEG: turns the polygon.
// --projection: an orthographic, equirectangular (lat-long panorama) or equidistant fisheye camera instead of the perspective pinhole (FCamera::SetProjection), from the scene
// camera's position and axes.  --ortho-scale S: the width of the orthographic view in units of the camera's right vector (default 1); --fisheye-fov DEG: the fisheye's field
// of view, (0, 360], default 180, reached at the half-diagonal, half-width or half-height of the film (--fisheye-fit).  With --hdr --format hdr an equirect render is a map
// --envmap takes.  Not together with --aperture.
// --smooth: vertex normals for the scenes' meshes (FSmoothing; lights excepted): `file` takes the OBJ's vn, a number computes them with that crease angle in degrees.
// --estimator mis: next-event estimation and the BSDF sample weighted against each other (FScene::SetEstimator(JP_ESTIMATOR_MIS)); implies --light-sampling power.
// nee (default): the reference's estimator.
// --envmap FILE: light the scene with a lat-long image (PFM, Radiance .hdr, binary PPM, BMP; FScene::SetEnvironmentMap): the scene script's background
// becomes the tint (S, S, S), S = 1 unless --envmap-scale says otherwise; --envmap-up: the map's up axis (default y, the scenes' up); power sampling is implied.
// --light-sampling power: one light per bounce, picked by power (FScene::SetLightSampling(JP_LIGHTS_POWER_ONE)); all (default): every light at every bounce.
// --denoise: the edge-avoiding filter on the rendered film (FFilm::RequestDenoise); --guide-spp: camera samples per pixel of its guides (default 8,
// 1 .. 1024); --aov: the guides as images PREFIX_albedo, PREFIX_normal (n * 0.5 + 0.5), PREFIX_depth (t / max t) in the chosen format.
// --denoise variance: the variance-guided filter on a variance render instead (FDenoiseOptions::varianceGuided; needs spp >= 2); --aov then, and without --denoise
// at spp >= 2, also writes PREFIX_variance (v / max v), the per-pixel variance of the film's mean luminance (FFilm::RequestVariance).
// --adaptive THRESHOLD: adaptive sampling (FFilm::SetAdaptive): a pixel stops once the relative standard error of its mean luminance is below THRESHOLD; spp
// is the most a pixel takes, --min-spp (default 8) what every pixel takes first, --spp-step (default 8) what a pass adds; --no-adaptive-dilate tests each pixel
// alone instead of with its 3 x 3 neighbourhood.  --aov then also writes PREFIX_samples (n / spp) and PREFIX_variance.  The path integrator; the image is encoded
// on the host (no --tonemap / --exposure with it); with --denoise it takes the variance-guided filter.
// sceneid 0 = Cornell box, 1 = bunny scene; spp defaults to 50, the film to 1024 x 1024, the output to
// <scene name>_<spp>.bmp, as in the reference.  The scene scripts are the calls of main.cc:13-111; the meshes are
// read from DIR/cornellbox/{light,floor,shortbox,tallbox,left,right}.obj and DIR/bunny/bunny.obj (the reference
// reads scene\cornellbox\... relative to the working directory; its assets are not in its repository --
// `python -m jet_pbrt_amd.scenes DIR` writes the synthetic stand-ins).
#include "jetpbrt.h"

#include <cstdlib>
#include <cstring>

using namespace jetpbrt;

static FColor LightRadiance()                                    // main.cc:35
{
	auto V = [](Float a, Float b, Float c) { return FVector3(a, b, c); };
	FVector3 r = V(0.747f + 0.058f, 0.747f + 0.258f, 0.747f) * 8.0f + V(0.740f + 0.287f, 0.740f + 0.160f, 0.740f) * 15.6f + V(0.737f + 0.642f, 0.737f + 0.159f, 0.737f) * 18.4f;
	return FColor(r.x, r.y, r.z);
}

// nmap (--normal-map): the floor gets a material of its own that carries it; *floorHasUV tells whether the floor mesh has texture coordinates at all
static std::shared_ptr<FScene> create_cornellbox_scene(const FVector2& filmsize, const std::string& dir, const FColor* background = nullptr, const FSmoothing& sm = FSmoothing(),
                                                       const std::shared_ptr<FNormalMap>& nmap = nullptr, float nstrength = 1.f, bool* floorHasUV = nullptr, const std::shared_ptr<FTexture>& floorTex = nullptr)   // main.cc:13-62; background: --envmap's tint; sm: --smooth
{
	const FPoint3 lookfrom(278, 273, 960), lookat(278, 273, 0);
	std::shared_ptr<FScene> scene = std::make_shared<FScene>("cornell_box_scene");
	scene->CreateCamera<FCamera>(lookfrom, Normalize(lookat - lookfrom), FVector3(0, 1, 0), (Float)60.0, filmsize);
	scene->CreateLight<FEnvironmentLight>(FPoint3(0, 0, 0), 1, background ? *background : FColor(0.f, 0.f, 0.f));
	std::shared_ptr<FMaterial> red = scene->CreateMaterial<FMatteMaterial>(FColor(0.63f, 0.065f, 0.05f));
	std::shared_ptr<FMaterial> green = scene->CreateMaterial<FMatteMaterial>(FColor(0.14f, 0.45f, 0.091f));
	std::shared_ptr<FMaterial> white = scene->CreateMaterial<FMatteMaterial>(FColor(0.725f, 0.71f, 0.68f));
	std::shared_ptr<FMaterial> golden = scene->CreateMaterial<FMetalMaterial>(FColor(0.18f, 0.15f, 0.81f), FColor(0.11f, 0.11f, 0.11f), 0.2f, 0.2f, false);
	std::shared_ptr<FMaterial> mat_light = scene->CreateMaterial<FMatteMaterial>(FColor(0.65f, 0.65f, 0.65f));
	const std::string d = dir + "/cornellbox/";
	scene->CreateAreaLights(1, LightRadiance(), scene->CreateTriangleMesh((d + "light.obj").c_str(), true, true), mat_light);
	const std::vector<std::shared_ptr<FShape>> floorMesh = scene->CreateTriangleMesh((d + "floor.obj").c_str(), true, true, FVector3(0, 0, 0), 1.f, sm);
	std::shared_ptr<FMaterial> floorMat = white;
	if (floorTex) floorMat = scene->CreateMaterial<FMatteMaterial>(floorTex);     // --floor-texture: a material of the floor's own
	if (nmap)
	{
		if (!floorTex) floorMat = scene->CreateMaterial<FMatteMaterial>(FColor(0.725f, 0.71f, 0.68f));
		floorMat->normalMap = nmap; floorMat->normalStrength = nstrength;
		bool uv = floorMesh.empty();                                  // (a mesh that did not load is reported as such, below)
		for (auto& sh : floorMesh) { const FTriangle* t = static_cast<const FTriangle*>(sh.get()); if (t->uv0.x != t->uv1.x || t->uv0.y != t->uv1.y || t->uv0.x != t->uv2.x || t->uv0.y != t->uv2.y) uv = true; }
		if (floorHasUV) *floorHasUV = uv;
	}
	scene->CreatePrimitives(floorMesh, floorMat);
	scene->CreatePrimitives(scene->CreateTriangleMesh((d + "shortbox.obj").c_str(), true, true, FVector3(0, 0, 0), 1.f, sm), white);
	scene->CreatePrimitives(scene->CreateTriangleMesh((d + "tallbox.obj").c_str(), true, true, FVector3(0, 0, 0), 1.f, sm), golden);
	scene->CreatePrimitives(scene->CreateTriangleMesh((d + "left.obj").c_str(), true, true, FVector3(0, 0, 0), 1.f, sm), red);
	scene->CreatePrimitives(scene->CreateTriangleMesh((d + "right.obj").c_str(), true, true, FVector3(0, 0, 0), 1.f, sm), green);
	scene->Preprocess();
	return scene;
}

static std::shared_ptr<FScene> create_bunny_scene(const FVector2& filmsize, const std::string& dir, const FColor* background = nullptr, const FSmoothing& sm = FSmoothing(),
                                                  const std::shared_ptr<FNormalMap>& nmap = nullptr, float nstrength = 1.f, const std::shared_ptr<FTexture>& floorTex = nullptr)        // main.cc:64-111
{
	const FPoint3 lookfrom(-300, 300, -300), lookat(0, 0, 0);
	std::shared_ptr<FScene> scene = std::make_shared<FScene>("bunny_scene");
	scene->CreateCamera<FCamera>(lookfrom, Normalize(lookat - lookfrom), FVector3(0, 1, 0), (Float)60.0, filmsize);
	scene->CreateLight<FEnvironmentLight>(FPoint3(0, 0, 0), 1, background ? *background : FColor(0.1f, 0.1f, 0.5f));
	std::shared_ptr<FMaterial> red = scene->CreateMaterial<FMatteMaterial>(FColor(0.63f, 0.065f, 0.05f));
	std::shared_ptr<FMaterial> green = scene->CreateMaterial<FMatteMaterial>(FColor(0.14f, 0.45f, 0.091f));
	scene->CreateMaterial<FMatteMaterial>(FColor(0.725f, 0.71f, 0.68f));
	std::shared_ptr<FMaterial> mat_light = scene->CreateMaterial<FMatteMaterial>(FColor(0.65f, 0.65f, 0.65f));
	std::shared_ptr<FShape> light = scene->CreateShape<FRectangle>(FRectangle::FromXZ(-100, 100, -100, 100, 350, true));
	scene->CreateAreaLight(1, LightRadiance(), light, mat_light);
	std::shared_ptr<FShape> floor = scene->CreateShape<FRectangle>(FRectangle::FromXZ(-200, 200, -200, 200, 0));
	if (nmap) { green->normalMap = nmap; green->normalStrength = nstrength; }     // (green is the floor's alone)
	if (floorTex) green->texture = floorTex;
	scene->CreatePrimitive(floor.get(), green.get(), (const FAreaLight*)nullptr);
	const std::string obj = dir + "/bunny/bunny.obj";
	scene->CreatePrimitives(scene->CreateTriangleMesh(obj.c_str(), true, true, FVector3(0, 0, 0), 500.f, sm), red);
	std::shared_ptr<FMaterial> plastic = scene->CreateMaterial<FPlasticMaterial>(FColor(0.35f, 0.12f, 0.48f), FColor(1) - FColor(0.35f, 0.12f, 0.48f), 0.1f, false);
	scene->CreatePrimitives(scene->CreateTriangleMesh(obj.c_str(), true, true, FVector3(-100, 0, -100), 500.f, sm), plastic);
	std::shared_ptr<FMaterial> golden = scene->CreateMaterial<FMetalMaterial>(FColor(0.18f, 0.15f, 0.81f), FColor(0.11f, 0.11f, 0.11f), 0.2f, 0.2f, false);
	scene->CreatePrimitives(scene->CreateTriangleMesh(obj.c_str(), true, true, FVector3(0, 0, -100), 500.f, sm), golden);
	std::shared_ptr<FMaterial> glass = scene->CreateMaterial<FGlassMaterial>(1.5f, FColor(0.98f), FColor(0.98f));
	scene->CreatePrimitives(scene->CreateTriangleMesh(obj.c_str(), true, true, FVector3(-100, 0, 0), 500.f, sm), glass);
	scene->Preprocess();
	return scene;
}

int main(int argc, char* argv[])
{
	int width = 1024, height = 1024, samples_per_pixel = 50;     // main.cc:115,119
	std::string assets = "scene", out, format = "bmp", integratorName = "path";
	bool adaptive = false, adaptiveDilate = true; float adaptiveThreshold = 0.f; int minSpp = 8, sppStep = 8;
	bool denoise = false, denoiseVariance = false; int guideSpp = 8; std::string aov; int lightSampling = JP_LIGHTS_ALL, estimator = JP_ESTIMATOR_NEE;
	std::string envmap; int envUp = JP_ENV_UP_Y; float envScale = 1.f;
	FSmoothing smoothing;
	std::string normalMap; float normalStrength = 1.f, normalFromHeight = 0.f; bool fromHeight = false;
	bool hdr = false, haveToneMap = false; float sampleClamp = 0.f; FToneMap toneMap;
	FTexSampling texSampling, normalSampling; bool haveTexSampling = false, haveNormalSampling = false;
	bool textureMip = false; float mipFootprint = 0.f, mipBounceSpread = 0.f;
	int floorTexture = JP_PROC_NONE, floorOctaves = 0; float floorScale = 0.02f; bool floorAntialias = true, floorOptions = false;
	int projection = JP_PROJ_PERSPECTIVE, fisheyeFit = JP_FIT_DIAGONAL; float orthoScale = 0.f, fisheyeFov = 0.f;
	float aperture = 0.f, focus = 1.f, focusX = 0.f, focusY = 0.f, apertureRotation = 0.f; int blades = 0; bool focusPixel = false;
	fprintf(stderr, "pbrt.exe  sceneid   spp\n");                 // main.cc:121
	fprintf(stderr, "          [width height] [--assets DIR] [--out NAME] [--format bmp|ppm|hdr] [--adaptive THRESHOLD [--min-spp N] [--spp-step N] [--no-adaptive-dilate]] [--denoise [variance]] [--guide-spp N] [--aov PREFIX] [--light-sampling all|power] [--estimator nee|mis] [--envmap FILE [--envmap-up y|z] [--envmap-scale S]] [--smooth file|DEG]\n");
	fprintf(stderr, "          [--aperture R [--focus D | --focus-pixel X Y] [--blades N] [--aperture-rotation DEG]]\n");
	fprintf(stderr, "          [--projection ortho|equirect|fisheye [--ortho-scale S] [--fisheye-fov DEG] [--fisheye-fit diagonal|width|height]]\n");
	fprintf(stderr, "          [--normal-map FILE [--normal-strength S] [--normal-from-height SCALE]]\n");
	fprintf(stderr, "          [--hdr] [--sample-clamp C] [--tonemap clamp|reinhard|aces|hable] [--exposure EV|auto] [--white W]\n");
	fprintf(stderr, "          [--texture-wrap clamp|repeat|mirror] [--texture-filter nearest|bilinear] [--texture-tile SU SV] [--normal-wrap clamp|repeat] [--normal-tile SU SV]\n");
	fprintf(stderr, "          [--texture-mip [--mip-footprint S] [--mip-bounce-spread RAD]]\n");
	fprintf(stderr, "          [--floor-texture noise|fbm|turbulence|marble|checker [--floor-texture-scale S] [--floor-texture-octaves N] [--no-texture-antialias]]\n");
	std::vector<const char*> pos;
	for (int i = 1; i < argc; i++)
	{
		if (!strcmp(argv[i], "--assets") && i + 1 < argc) assets = argv[++i];
		else if (!strcmp(argv[i], "--out") && i + 1 < argc) out = argv[++i];
		else if (!strcmp(argv[i], "--format") && i + 1 < argc) format = argv[++i];
		else if (!strcmp(argv[i], "--device-bvh")) setenv("JETPBRT_DEVICE_BVH", "1", 1);   // FScene::deviceBuild for the scenes created below
		else if (!strcmp(argv[i], "--integrator") && i + 1 < argc) integratorName = argv[++i];
		else if (!strcmp(argv[i], "--reference-tree")) setenv("JETPBRT_REFERENCE_TREE", "1", 1);   // FScene::referenceTree: the reference's own BVH and traversal semantics
		else if (!strcmp(argv[i], "--reference-tree=certified")) setenv("JETPBRT_REFERENCE_TREE", "2", 1);   // ... with the certified walk (FScene::certifiedWalk)
		else if (!strcmp(argv[i], "--denoise")) { denoise = true; if (i + 1 < argc && !strcmp(argv[i + 1], "variance")) { denoiseVariance = true; i++; } }
		else if (!strcmp(argv[i], "--adaptive") && i + 1 < argc) { adaptive = true; adaptiveThreshold = (float)atof(argv[++i]); if (!(adaptiveThreshold >= 0.f) || !std::isfinite(adaptiveThreshold)) { fprintf(stderr, "--adaptive THRESHOLD must be finite and >= 0\n"); return 5; } }
		else if (!strcmp(argv[i], "--min-spp") && i + 1 < argc) { minSpp = atoi(argv[++i]); if (minSpp < 2) { fprintf(stderr, "--min-spp must be >= 2\n"); return 5; } }
		else if (!strcmp(argv[i], "--spp-step") && i + 1 < argc) { sppStep = atoi(argv[++i]); if (sppStep < 1) { fprintf(stderr, "--spp-step must be >= 1\n"); return 5; } }
		else if (!strcmp(argv[i], "--no-adaptive-dilate")) adaptiveDilate = false;
		else if (!strcmp(argv[i], "--guide-spp") && i + 1 < argc) { guideSpp = atoi(argv[++i]); if (guideSpp < 1 || guideSpp > 1024) { fprintf(stderr, "--guide-spp must be 1 .. 1024\n"); return 5; } }
		else if (!strcmp(argv[i], "--aov") && i + 1 < argc) aov = argv[++i];
		else if (!strcmp(argv[i], "--light-sampling") && i + 1 < argc)
		{
			const char* m = argv[++i];
			if (!strcmp(m, "power")) lightSampling = JP_LIGHTS_POWER_ONE; else if (!strcmp(m, "all")) lightSampling = JP_LIGHTS_ALL;
			else { fprintf(stderr, "--light-sampling must be all or power\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--estimator") && i + 1 < argc)
		{
			const char* m = argv[++i];
			if (!strcmp(m, "mis")) estimator = JP_ESTIMATOR_MIS; else if (!strcmp(m, "nee")) estimator = JP_ESTIMATOR_NEE;
			else { fprintf(stderr, "--estimator must be nee or mis\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--envmap") && i + 1 < argc) envmap = argv[++i];
		else if (!strcmp(argv[i], "--envmap-up") && i + 1 < argc)
		{
			const char* m = argv[++i];
			if (!strcmp(m, "y")) envUp = JP_ENV_UP_Y; else if (!strcmp(m, "z")) envUp = JP_ENV_UP_Z;
			else { fprintf(stderr, "--envmap-up must be y or z\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--envmap-scale") && i + 1 < argc) { envScale = (float)atof(argv[++i]); if (!(envScale >= 0.f) || !std::isfinite(envScale)) { fprintf(stderr, "--envmap-scale must be a number >= 0\n"); return 5; } }
		else if (!strcmp(argv[i], "--smooth") && i + 1 < argc)
		{
			const char* m = argv[++i]; char* e = nullptr; const float a = strtof(m, &e);
			if (!strcmp(m, "file")) smoothing = FSmoothing::File();
			else if (e != m && *e == 0 && a >= 0.f && a <= 180.f) smoothing = FSmoothing::Angle(a);
			else { fprintf(stderr, "--smooth must be file or an angle of 0 .. 180 degrees\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--aperture") && i + 1 < argc) { aperture = (float)atof(argv[++i]); if (!(aperture >= 0.f) || !std::isfinite(aperture)) { fprintf(stderr, "--aperture must be a number >= 0\n"); return 5; } }
		else if (!strcmp(argv[i], "--focus") && i + 1 < argc) { focus = (float)atof(argv[++i]); focusPixel = false; if (!(focus > 0.f) || !std::isfinite(focus)) { fprintf(stderr, "--focus must be a number > 0\n"); return 5; } }
		else if (!strcmp(argv[i], "--focus-pixel") && i + 2 < argc) { focusX = (float)atof(argv[i + 1]); focusY = (float)atof(argv[i + 2]); i += 2; focusPixel = true; if (!std::isfinite(focusX) || !std::isfinite(focusY)) { fprintf(stderr, "--focus-pixel takes two numbers\n"); return 5; } }
		else if (!strcmp(argv[i], "--blades") && i + 1 < argc) { blades = atoi(argv[++i]); if (blades != 0 && (blades < 3 || blades > 16)) { fprintf(stderr, "--blades must be 0 (a disk) or 3 .. 16\n"); return 5; } }
		else if (!strcmp(argv[i], "--aperture-rotation") && i + 1 < argc) { apertureRotation = (float)atof(argv[++i]); if (!std::isfinite(apertureRotation)) { fprintf(stderr, "--aperture-rotation must be a number\n"); return 5; } }
		else if (!strcmp(argv[i], "--projection") && i + 1 < argc)
		{
			const char* m = argv[++i];
			if (!strcmp(m, "ortho")) projection = JP_PROJ_ORTHOGRAPHIC; else if (!strcmp(m, "equirect")) projection = JP_PROJ_EQUIRECT;
			else if (!strcmp(m, "fisheye")) projection = JP_PROJ_FISHEYE; else if (!strcmp(m, "perspective")) projection = JP_PROJ_PERSPECTIVE;
			else { fprintf(stderr, "--projection must be ortho, equirect, fisheye or perspective\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--ortho-scale") && i + 1 < argc) orthoScale = (float)atof(argv[++i]);      // (checked with the projection below, by the library)
		else if (!strcmp(argv[i], "--fisheye-fov") && i + 1 < argc) fisheyeFov = (float)atof(argv[++i]);
		else if (!strcmp(argv[i], "--fisheye-fit") && i + 1 < argc)
		{
			const char* m = argv[++i];
			if (!strcmp(m, "diagonal")) fisheyeFit = JP_FIT_DIAGONAL; else if (!strcmp(m, "width")) fisheyeFit = JP_FIT_WIDTH; else if (!strcmp(m, "height")) fisheyeFit = JP_FIT_HEIGHT;
			else { fprintf(stderr, "--fisheye-fit must be diagonal, width or height\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--normal-map") && i + 1 < argc) normalMap = argv[++i];
		else if (!strcmp(argv[i], "--normal-strength") && i + 1 < argc) { normalStrength = (float)atof(argv[++i]); if (!std::isfinite(normalStrength)) { fprintf(stderr, "--normal-strength must be a number\n"); return 5; } }
		else if (!strcmp(argv[i], "--normal-from-height") && i + 1 < argc) { normalFromHeight = (float)atof(argv[++i]); fromHeight = true; if (!std::isfinite(normalFromHeight)) { fprintf(stderr, "--normal-from-height must be a number\n"); return 5; } }
		else if (!strcmp(argv[i], "--texture-wrap") && i + 1 < argc)
		{
			const char* m = argv[++i]; haveTexSampling = true;
			if (!strcmp(m, "clamp")) texSampling.wrapU = texSampling.wrapV = EWrap::Clamp; else if (!strcmp(m, "repeat")) texSampling.wrapU = texSampling.wrapV = EWrap::Repeat;
			else if (!strcmp(m, "mirror")) texSampling.wrapU = texSampling.wrapV = EWrap::Mirror;
			else { fprintf(stderr, "--texture-wrap must be clamp, repeat or mirror\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--texture-filter") && i + 1 < argc)
		{
			const char* m = argv[++i]; haveTexSampling = true;
			if (!strcmp(m, "nearest")) texSampling.filter = EFilter::Nearest; else if (!strcmp(m, "bilinear")) texSampling.filter = EFilter::Bilinear;
			else { fprintf(stderr, "--texture-filter must be nearest or bilinear\n"); return 5; }
		}
		else if ((!strcmp(argv[i], "--texture-tile") || !strcmp(argv[i], "--normal-tile")) && i + 2 < argc)
		{
			const bool normal = !strcmp(argv[i], "--normal-tile");
			char *e0 = nullptr, *e1 = nullptr; const float su = strtof(argv[i + 1], &e0), sv = strtof(argv[i + 2], &e1);
			if (e0 == argv[i + 1] || *e0 || e1 == argv[i + 2] || *e1 || !(su > 0.f) || !(sv > 0.f) || !std::isfinite(su) || !std::isfinite(sv)) { fprintf(stderr, "%s takes two numbers > 0\n", argv[i]); return 5; }
			FTexSampling& s = normal ? normalSampling : texSampling; s.scaleU = su; s.scaleV = sv; (normal ? haveNormalSampling : haveTexSampling) = true;
			i += 2;
		}
		else if (!strcmp(argv[i], "--normal-wrap") && i + 1 < argc)
		{
			const char* m = argv[++i]; haveNormalSampling = true;
			if (!strcmp(m, "clamp")) normalSampling.wrapU = normalSampling.wrapV = EWrap::Clamp; else if (!strcmp(m, "repeat")) normalSampling.wrapU = normalSampling.wrapV = EWrap::Repeat;
			else { fprintf(stderr, "--normal-wrap must be clamp or repeat\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--texture-mip")) textureMip = true;
		else if (!strcmp(argv[i], "--floor-texture") && i + 1 < argc)
		{
			const char* m = argv[++i];
			if (!strcmp(m, "noise")) floorTexture = JP_PROC_NOISE; else if (!strcmp(m, "fbm")) floorTexture = JP_PROC_FBM; else if (!strcmp(m, "turbulence")) floorTexture = JP_PROC_TURBULENCE;
			else if (!strcmp(m, "marble")) floorTexture = JP_PROC_MARBLE; else if (!strcmp(m, "checker")) floorTexture = JP_PROC_CHECKER_AA;
			else { fprintf(stderr, "--floor-texture must be noise, fbm, turbulence, marble or checker\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--floor-texture-scale") && i + 1 < argc)
		{
			char* e = nullptr; floorScale = strtof(argv[i + 1], &e); floorOptions = true;
			if (e == argv[i + 1] || *e || !(floorScale > 0.f) || !std::isfinite(floorScale)) { fprintf(stderr, "--floor-texture-scale takes a number > 0\n"); return 5; }
			i++;
		}
		else if (!strcmp(argv[i], "--floor-texture-octaves") && i + 1 < argc)
		{
			char* e = nullptr; const long v = strtol(argv[i + 1], &e, 10); floorOptions = true;
			if (e == argv[i + 1] || *e || v < 1 || v > 12) { fprintf(stderr, "--floor-texture-octaves takes 1 .. 12\n"); return 5; }
			floorOctaves = (int)v; i++;
		}
		else if (!strcmp(argv[i], "--no-texture-antialias")) { floorAntialias = false; floorOptions = true; }
		else if (!strncmp(argv[i], "--floor-texture", 15)) { fprintf(stderr, "%s: missing value\n", argv[i]); return 5; }
		else if ((!strcmp(argv[i], "--mip-footprint") || !strcmp(argv[i], "--mip-bounce-spread")) && i + 1 < argc)
		{
			char* e = nullptr; const float v = strtof(argv[i + 1], &e);
			if (e == argv[i + 1] || *e || !(v > 0.f) || !std::isfinite(v)) { fprintf(stderr, "%s takes a number > 0\n", argv[i]); return 5; }
			(!strcmp(argv[i], "--mip-footprint") ? mipFootprint : mipBounceSpread) = v; i++;
		}
		else if (!strcmp(argv[i], "--mip-footprint") || !strcmp(argv[i], "--mip-bounce-spread")) { fprintf(stderr, "%s: missing value\n", argv[i]); return 5; }
		else if (!strncmp(argv[i], "--texture-", 10) || !strcmp(argv[i], "--normal-wrap") || !strcmp(argv[i], "--normal-tile")) { fprintf(stderr, "%s: missing value\n", argv[i]); return 5; }
		else if (!strcmp(argv[i], "--hdr")) hdr = true;
		else if (!strcmp(argv[i], "--sample-clamp") && i + 1 < argc) { sampleClamp = (float)atof(argv[++i]); if (!(sampleClamp >= 0.f) || !std::isfinite(sampleClamp)) { fprintf(stderr, "--sample-clamp must be a number >= 0\n"); return 5; } }
		else if (!strcmp(argv[i], "--tonemap") && i + 1 < argc)
		{
			const char* m = argv[++i]; haveToneMap = true;
			if (!strcmp(m, "clamp")) toneMap.curve = JP_CURVE_CLAMP; else if (!strcmp(m, "reinhard")) toneMap.curve = JP_CURVE_REINHARD;
			else if (!strcmp(m, "aces")) toneMap.curve = JP_CURVE_ACES; else if (!strcmp(m, "hable")) toneMap.curve = JP_CURVE_HABLE;
			else { fprintf(stderr, "--tonemap must be clamp, reinhard, aces or hable\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--exposure") && i + 1 < argc)
		{
			const char* m = argv[++i]; char* e = nullptr; const float v = strtof(m, &e); haveToneMap = true;
			if (!strcmp(m, "auto")) toneMap.autoExposure = true;
			else if (e != m && *e == 0 && std::isfinite(v)) { toneMap.autoExposure = false; toneMap.ev = v; }
			else { fprintf(stderr, "--exposure must be a number (EV) or auto\n"); return 5; }
		}
		else if (!strcmp(argv[i], "--white") && i + 1 < argc) { toneMap.white = (float)atof(argv[++i]); haveToneMap = true; if (!(toneMap.white > 0.f) || !std::isfinite(toneMap.white)) { fprintf(stderr, "--white must be a number > 0\n"); return 5; } }
		else pos.push_back(argv[i]);
	}
	if ((orthoScale != 0.f || fisheyeFov != 0.f || fisheyeFit != JP_FIT_DIAGONAL) && projection == JP_PROJ_PERSPECTIVE) { fprintf(stderr, "--ortho-scale / --fisheye-fov / --fisheye-fit need --projection\n"); return 5; }
	if (projection != JP_PROJ_PERSPECTIVE)
	{   // the library's own validation (jp_check_projection: pure host code), before anything is loaded
		if (aperture > 0.f) { fprintf(stderr, "--projection and --aperture exclude each other (a lens belongs to the perspective camera)\n"); return 5; }
		FCamera probe(FVector3(0, 0, 0), FVector3(0, 0, -1), FVector3(0, 1, 0), 45.f, FVector2(1, 1));
		probe.SetProjection(projection, orthoScale, fisheyeFov, fisheyeFit);
		std::string msg;
		if (!probe.CheckProjection(&msg)) { fprintf(stderr, "--projection: %s\n", msg.c_str()); return 5; }
	}
	if (pos.empty()) return 0;                                    // main.cc:122-125
	const int sceneId = atoi(pos[0]);
	if (pos.size() > 1) { int spp = atoi(pos[1]); if (spp > 0) samples_per_pixel = spp; }
	if (pos.size() > 3) { int w = atoi(pos[2]), h = atoi(pos[3]); if (w > 0 && h > 0) { width = w; height = h; } }
	FFilm film(width, height);
	std::shared_ptr<FEnvironmentMap> map;
	if (!envmap.empty())
	{
		std::string err;
		map = FEnvironmentMap::FromFile(envmap.c_str(), &err);
		if (!map) { fprintf(stderr, "--envmap %s: %s\n", envmap.c_str(), err.c_str()); return 5; }
	}
	std::shared_ptr<FNormalMap> nmap;
	if (!normalMap.empty())
	{
		nmap = FNormalMap::FromFile(normalMap.c_str());
		if (!nmap) { fprintf(stderr, "--normal-map %s: not a binary PPM or an uncompressed BMP of 1 .. 16384 texels per side\n", normalMap.c_str()); return 5; }
		if (fromHeight)
		{   // the red channel as the height
			std::vector<uint8_t> grey((size_t)nmap->width * nmap->height);
			for (size_t k = 0; k < grey.size(); k++) grey[k] = nmap->data[3 * k];
			nmap = FNormalMap::FromHeight(grey.data(), nmap->width, nmap->height, normalFromHeight);
		}
		if (haveNormalSampling) nmap->SetSampling(normalSampling);
	}
	bool floorHasUV = true;
	const FColor tint(envScale, envScale, envScale);
	if (floorOptions && floorTexture == JP_PROC_NONE) { fprintf(stderr, "--floor-texture-scale / --floor-texture-octaves / --no-texture-antialias need --floor-texture\n"); return 5; }
	std::shared_ptr<FTexture> floorTex;
	if (floorTexture != JP_PROC_NONE)
	{   // world space, the same scale on every axis; the floor's own colour at t = 0, a dark slate at t = 1
		const float m[12] = { floorScale, 0, 0, 0, 0, floorScale, 0, 0, 0, 0, floorScale, 0 };
		floorTex = std::make_shared<FProceduralTexture>(floorTexture, FColor(0.2f, 0.2f, 0.25f), FColor(0.725f, 0.71f, 0.68f), m, floorOctaves, 0.f, floorAntialias);
	}
	std::shared_ptr<FScene> scene;
	switch (sceneId)
	{
	case 0: scene = create_cornellbox_scene(film.GetResolution(), assets, map ? &tint : nullptr, smoothing, nmap, normalStrength, &floorHasUV, floorTex); break;
	case 1: scene = create_bunny_scene(film.GetResolution(), assets, map ? &tint : nullptr, smoothing, nmap, normalStrength, floorTex); break;
	default: return 0;
	}
	if (nmap && !floorHasUV) { fprintf(stderr, "--normal-map: %s/cornellbox/floor.obj has no texture coordinates (vt), so nothing would be mapped\n", assets.c_str()); return 5; }
	if (map) scene->SetEnvironmentMap(map, envUp);
	if ((mipFootprint != 0.f || mipBounceSpread != 0.f) && !textureMip) { fprintf(stderr, "--mip-footprint / --mip-bounce-spread need --texture-mip\n"); return 5; }
	if (textureMip) { scene->SetTextureMipmapDefault(true); scene->mipFootprintScale = mipFootprint; scene->mipBounceSpread = mipBounceSpread; }
	if (haveTexSampling) scene->SetTextureSamplingDefault(texSampling);   // every image texture without a sampling of its own (the scene is flattened at Render)
	fprintf(stderr, "current scene: %s\n", scene->NameStr());
	scene->SetLightSampling(estimator == JP_ESTIMATOR_MIS ? JP_LIGHTS_POWER_ONE : lightSampling);
	scene->SetEstimator(estimator);
	if (aperture > 0.f && scene->camera)
	{
		scene->camera->SetLens(aperture, focus, blades, apertureRotation);
		if (focusPixel) scene->camera->FocusAt(focusX, focusY);
	}
	if (projection != JP_PROJ_PERSPECTIVE && scene->camera) scene->camera->SetProjection(projection, orthoScale, fisheyeFov, fisheyeFit);
	if (scene->primitives.empty()) { fprintf(stderr, "no geometry loaded from %s\n", assets.c_str()); return 2; }
	std::shared_ptr<FSampler> sampler = std::make_shared<FRandomSampler>(samples_per_pixel);
	// main.cc:154 constructs FPathIntegratorIteration(5); the commented-out alternatives of main.cc:150-153 are selectable here
	std::unique_ptr<FGpuPathIntegrator> integrator;
	if (integratorName == "whitted") integrator.reset(new FWhittedIntegrator(5));
	else if (integratorName == "debug") integrator.reset(new FDebugIntegrator());
	else if (integratorName == "recursive") integrator.reset(new FPathIntegratorRecursive(5));
	else integrator.reset(new FPathIntegratorIteration(5));
	if (adaptive && haveToneMap) { fprintf(stderr, "--adaptive delivers the fp32 film: no --tonemap / --exposure / --white with it\n"); return 5; }
	if (adaptive && denoise) denoiseVariance = true;              // (the adaptive render's own variance plane feeds the filter)
	if (adaptive) film.SetAdaptive(adaptiveThreshold, std::min(minSpp, samples_per_pixel), sppStep, adaptiveDilate);
	if (format != "hdr" && !adaptive) film.RequestDeviceLDR(true);             // BMP / PPM: gamma_encoding runs on the GPU, 3 bytes per pixel come back
	if (hdr) film.SetHDR();
	if (sampleClamp > 0.f) film.SetSampleClamp(sampleClamp);
	if (haveToneMap) film.SetToneMap(toneMap);                    // (turns HDR on)
	if (denoiseVariance) { FDenoiseOptions o; o.varianceGuided = true; film.RequestDenoise(guideSpp, o); }
	else if (denoise) film.RequestDenoise(guideSpp);
	else if (!aov.empty()) { film.RequestGuides(guideSpp); if (samples_per_pixel >= 2) film.RequestVariance(); }
	integrator->Render(scene.get(), sampler.get(), &film, 16);    // main.cc:156
	if (integrator->LastStatus() != JP_OK) return 3;              // no GPU / no library: fail loudly, nothing is written
	if (aperture > 0.f && scene->camera) fprintf(stderr, "lens: aperture %g, focus distance %g%s\n", aperture, scene->camera->LastFocus(), focusPixel ? " (found at the focus pixel)" : "");
	if (haveToneMap) fprintf(stderr, "tone map: exposure scale %g\n", film.ToneMapScale());
	char fullname[512];
	snprintf(fullname, sizeof(fullname), "%s_%d", scene->NameStr(), samples_per_pixel);
	const std::string name = out.empty() ? fullname : out;
	const EImageType t = format == "ppm" ? EImageType::PPM : (format == "hdr" ? EImageType::HDR : EImageType::BMP);
	if (!aov.empty())
	{   // the guides through SaveAsImage: albedo as it is, normal n * 0.5 + 0.5, depth t / max t
		const size_t n = (size_t)width * height;
		Float zmax = 0; for (Float z : film.Depth()) zmax = z > zmax ? z : zmax;
		FFilm fa(width, height), fn(width, height), fz(width, height);
		for (size_t i = 0; i < n; i++)
		{
			const int x = (int)(i % width), y = (int)(i / width);
			fa(x, y) = film.Albedo()[i];
			const FVector3& v = film.Normal()[i]; fn(x, y) = FColor(v.x * 0.5f + 0.5f, v.y * 0.5f + 0.5f, v.z * 0.5f + 0.5f);
			const Float z = zmax > 0 ? film.Depth()[i] / zmax : 0; fz(x, y) = FColor(z, z, z);
		}
		if (!fa.SaveAsImage(aov + "_albedo", t) || !fn.SaveAsImage(aov + "_normal", t) || !fz.SaveAsImage(aov + "_depth", t)) return 4;
		if (film.SampleCounts().size() == n)
		{   // the samples each pixel took, n / spp
			FFilm fs(width, height);
			for (size_t i = 0; i < n; i++) { const Float v = (Float)film.SampleCounts()[i] / (Float)samples_per_pixel; fs((int)(i % width), (int)(i / width)) = FColor(v, v, v); }
			if (!fs.SaveAsImage(aov + "_samples", t)) return 4;
		}
		if (film.Variance().size() == n)
		{   // the variance plane, v / max v
			Float vmax = 0; for (Float v : film.Variance()) vmax = v > vmax ? v : vmax;
			FFilm fv(width, height);
			for (size_t i = 0; i < n; i++) { const Float v = vmax > 0 ? film.Variance()[i] / vmax : 0; fv((int)(i % width), (int)(i / width)) = FColor(v, v, v); }
			if (!fv.SaveAsImage(aov + "_variance", t)) return 4;
		}
	}
	return film.SaveAsImage(name, t) ? 0 : 4;                     // main.cc:160
}
