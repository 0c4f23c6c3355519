// tools/envmap_host_check.cpp -- the host half of environment maps as a stand-alone program for AddressSanitizer / UBSan: the table builder
// (csrc/jp_scene_host.h: check_environment_map, build_environment_table) and the float image readers (host/film_io.cc: ReadImagePFM, ReadImageHDR,
// FEnvironmentMap::FromFile) on good, truncated and malformed inputs.  These readers parse files from outside.  No context, no device: nothing is loaded
// into Python and nothing runs on a GPU.  From the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Wno-unused-value -Xarch_host -fsanitize=address,undefined -Iinclude -Ijet-pbrt_amd/csrc \
//         tools/envmap_host_check.cpp jet-pbrt_amd/host/film_io.cc -o envmap_host_check
//   ./envmap_host_check [scratch directory, default /tmp]        (prints one line per case, exit status 0 when every case did what it should)
#include "jp_common.h"
#include "jp_tex.h"
#include "jp_env.h"
#include "jp_xbsdf.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <thread>
#include <memory>
#include "jp_devmem.h"
#define JP_SHADE_TILE 8192              // as jp_kernels.hip defines it for k_shade
#include "jp_runtime.h"
#include "jp_scene_host.h"

namespace jetpbrt                         // host/film_io.cc (declared here: host/jetpbrt.h and the kernels' headers are not meant for one translation unit)
{
bool ReadImagePFM(const char* filename, std::vector<float>& rgb, int& width, int& height, std::string* error);
bool ReadImageHDR(const char* filename, std::vector<float>& rgb, int& width, int& height, std::string* error);
}

static int g_bad = 0;
static void expect(bool ok, const char* what) { printf("%-72s %s\n", what, ok ? "ok" : "FAILED"); if (!ok) g_bad++; }

static void write_file(const std::string& path, const std::string& bytes) { FILE* f = fopen(path.c_str(), "wb"); if (f) { fwrite(bytes.data(), 1, bytes.size(), f); fclose(f); } }

int main(int argc, char** argv)
{
	const std::string dir = argc > 1 ? argv[1] : "/tmp";
	// ---- table builder ---------------------------------------------------------------------------------------------------------------
	{
		const int W = 5, H = 3;
		std::vector<float> rgb(3 * W * H);
		for (size_t i = 0; i < rgb.size(); i++) rgb[i] = (float)((i * 7) % 11) * 0.25f;
		for (int c = 0; c < W; c++) rgb[3 * (W + c)] = rgb[3 * (W + c) + 1] = rgb[3 * (W + c) + 2] = 0.f;     // a black row
		JpEnvMap m; m.struct_bytes = (int32_t)sizeof(m); m.width = W; m.height = H; m.up_axis = JP_ENV_UP_Y; m.importance = 0; m.rgb = rgb.data();
		const float tint[3] = { 0.5f, 1.f, 2.f };
		EnvTables e;
		expect(build_environment_table(&m, tint, e) == JP_OK && e.texel.size() == (size_t)W * H && e.row_cos.size() == (size_t)H, "5 x 3 map: tables built");
		double psum = 0.0; bool black_unreachable = true;
		for (int t = 0; t < W * H; t++)
		{
			psum += (double)e.q[t] / (W * H); if (e.alias[t] != t) psum += 0.0;
			if (e.weight[t] == 0.0 && e.q[t] != 0.f) black_unreachable = false;
			if (e.weight[e.alias[t]] == 0.0 && e.q[t] != 1.f) black_unreachable = false;
		}
		expect(black_unreachable && e.n_selectable == W * (H - 1), "5 x 3 map: the black row is in no bin's reach");
		m.importance = -1;
		expect(build_environment_table(&m, tint, e) == JP_OK && e.n_selectable == W * H, "importance -1: every texel selectable");
		m.importance = 0; m.width = 0;
		expect(build_environment_table(&m, tint, e) == JP_ERR_INVALID_ARGUMENT, "width 0 refused");
		m.width = 4097;
		expect(build_environment_table(&m, tint, e) == JP_ERR_INVALID_ARGUMENT, "width 4097 refused");
		m.width = W; rgb[4] = -1.f;
		expect(build_environment_table(&m, tint, e) == JP_ERR_INVALID_ARGUMENT, "a negative texel refused");
		rgb[4] = NAN;
		expect(build_environment_table(&m, tint, e) == JP_ERR_INVALID_ARGUMENT, "a NaN texel refused");
		rgb[4] = INFINITY;
		expect(build_environment_table(&m, tint, e) == JP_ERR_INVALID_ARGUMENT, "an infinite texel refused");
		rgb[4] = 1.f; m.rgb = nullptr;
		expect(build_environment_table(&m, tint, e) == JP_ERR_INVALID_ARGUMENT, "null rgb refused");
		m.rgb = rgb.data(); m.struct_bytes = 8;
		expect(build_environment_table(&m, tint, e) == JP_ERR_INVALID_ARGUMENT, "short struct_bytes refused");
		m.struct_bytes = (int32_t)sizeof(m);
		std::vector<float> zero(3 * W * H, 0.f); m.rgb = zero.data();
		expect(build_environment_table(&m, tint, e) == JP_OK && e.total == 0.0 && e.n_selectable == 0 && e.texel[0].w == 0.f, "an all-black map: weight 0, pdf 0");
		// the largest map the definition allows on one side, thin: indices near 2^12 rows
		std::vector<float> tall(3 * 4096, 0.125f); m.rgb = tall.data(); m.width = 1; m.height = 4096;
		expect(build_environment_table(&m, tint, e) == JP_OK && e.n_selectable == 4096, "1 x 4096 map");
	}
	// ---- PFM ------------------------------------------------------------------------------------------------------------------------
	std::vector<float> rgb; int w = 0, h = 0; std::string err;
	{
		const float px[12] = { 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12 };       // 2 x 2, file order: bottom row first
		std::string body((const char*)px, sizeof(px));
		const std::string good = std::string("PF\n2 2\n-1.0\n") + body, p = dir + "/envmap_check.pfm";
		write_file(p, good);
		expect(jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err) && w == 2 && h == 2 && rgb[0] == 7.f && rgb[6] == 1.f, "PFM 2 x 2 little-endian, rows flipped");
		std::string be = body; for (size_t i = 0; i + 3 < be.size(); i += 4) { std::swap(be[i], be[i + 3]); std::swap(be[i + 1], be[i + 2]); }
		write_file(p, std::string("PF\n2 2\n1.0\n") + be);
		expect(jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err) && rgb[0] == 7.f && rgb[11] == 6.f, "PFM big-endian");
		write_file(p, std::string("Pf\n2 2\n-1.0\n") + body.substr(0, 16));
		expect(jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err) && rgb[0] == 3.f && rgb[1] == 3.f && rgb[9] == 2.f, "PFM grey");
		for (size_t cut : { (size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)6, (size_t)7, (size_t)11, (size_t)12, good.size() - 1, good.size() - 13 })
		{
			write_file(p, good.substr(0, cut));
			expect(!jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err) && rgb.empty(), ("PFM truncated at " + std::to_string(cut)).c_str());
		}
		write_file(p, std::string("PF\n0 2\n-1.0\n") + body); expect(!jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err), "PFM width 0 refused");
		write_file(p, std::string("PF\n99999 99999\n-1.0\n") + body); expect(!jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err), "PFM huge size refused");
		write_file(p, std::string("PF\n2 2\nabc\n") + body); expect(!jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err), "PFM bad scale refused");
		write_file(p, std::string("PF\n2 2\n0\n") + body); expect(!jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err), "PFM scale 0 refused");
		float neg[12]; std::memcpy(neg, px, sizeof(px)); neg[5] = -2.f;
		write_file(p, std::string("PF\n2 2\n-1.0\n") + std::string((const char*)neg, sizeof(neg))); expect(!jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err), "PFM negative value refused");
		neg[5] = NAN;
		write_file(p, std::string("PF\n2 2\n-1.0\n") + std::string((const char*)neg, sizeof(neg))); expect(!jetpbrt::ReadImagePFM(p.c_str(), rgb, w, h, &err), "PFM NaN refused");
		expect(!jetpbrt::ReadImagePFM((dir + "/envmap_check_missing.pfm").c_str(), rgb, w, h, &err), "PFM missing file refused");
		remove(p.c_str());
	}
	// ---- HDR ------------------------------------------------------------------------------------------------------------------------
	{
		const std::string head = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n", p = dir + "/envmap_check.hdr";
		const unsigned char flat[8] = { 128, 64, 32, 129, 0, 0, 0, 0 };      // (1, 0.5, 0.25), black
		const std::string good = head + "-Y 1 +X 2\n" + std::string((const char*)flat, 8);
		write_file(p, good);
		expect(jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err) && w == 2 && h == 1 && rgb[0] == 1.f && rgb[1] == 0.5f && rgb[2] == 0.25f && rgb[3] == 0.f, "HDR flat 2 x 1");
		for (size_t cut = 0; cut < good.size(); cut += 3)
		{
			write_file(p, good.substr(0, cut));
			expect(!jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err) && rgb.empty(), ("HDR truncated at " + std::to_string(cut)).c_str());
		}
		// a run-length encoded 8 x 1 scanline: per channel one run of 8
		std::string rle = head + "-Y 1 +X 8\n"; rle += std::string("\x02\x02\x00\x08", 4);
		const unsigned char ch[4] = { 128, 64, 32, 129 };
		for (int k = 0; k < 4; k++) { rle += (char)(128 + 8); rle += (char)ch[k]; }
		write_file(p, rle);
		expect(jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err) && w == 8 && rgb[21] == 1.f && rgb[23] == 0.25f, "HDR run-length encoded 8 x 1");
		std::string over = rle; over[over.size() - 2] = (char)(128 + 9);        // the last run overruns the scanline
		write_file(p, over); expect(!jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err), "HDR run past the scanline refused");
		std::string lit = head + "-Y 1 +X 8\n" + std::string("\x02\x02\x00\x08", 4) + std::string("\x08\x01\x02", 3);   // a literal of 8 with 2 bytes behind it
		write_file(p, lit); expect(!jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err), "HDR literal past the file refused");
		write_file(p, rle.substr(0, rle.size() - 1)); expect(!jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err), "HDR run-length data truncated refused");
		write_file(p, head + "+Y 1 +X 2\n" + std::string((const char*)flat, 8)); expect(!jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err), "HDR other orientation refused");
		write_file(p, head + "-Y 0 +X 2\n"); expect(!jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err), "HDR height 0 refused");
		write_file(p, head + "-Y 100000 +X 100000\n"); expect(!jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err), "HDR huge size refused");
		write_file(p, std::string("#?RADIANCE\n\n-Y 1 +X 2\n") + std::string((const char*)flat, 8)); expect(!jetpbrt::ReadImageHDR(p.c_str(), rgb, w, h, &err), "HDR without FORMAT refused");
		remove(p.c_str());
	}
	printf("%d case(s) failed\n", g_bad);
	return g_bad ? 1 : 0;
}
