// tools/mipmap_host_check.cpp -- include/jp_mipmap.h as a stand-alone program for AddressSanitizer / UBSan: the pyramid of images whose chains are heap blocks of exactly
// their texels (a source tap outside a level ends the program), the lookup above level 0 for every wrap_u x wrap_v on the edge set of coordinates times the edge set of
// footprints (1 + 2^-23, 2, 3, every power of two up to 2^127, 3e38), the level and the fraction of every such footprint, the footprint of degenerate areas and widths,
// and the cone's step on states that are not finite.  No context, no device: nothing is loaded into Python and nothing runs on a GPU.  From the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -Iinclude tools/mipmap_host_check.cpp -o mipmap_host_check
//   ./mipmap_host_check        (prints one line per image size, exit status 0 when every tap stayed inside its level and every value was defined)
#include "jp_mipmap.h"
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

int main()
{
	const int sizes[][2] = { { 1, 1 }, { 1, 5 }, { 5, 3 }, { 7, 2 }, { 8, 8 }, { 64, 64 }, { 16384, 1 }, { 3, 4097 } };
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	long long total = 0; int bad = 0;
	std::vector<float> rhos = { 1.0000001f, 1.5f, 2.f, 3.f, 3e38f, 3.4028235e38f };
	for (int k = 0; k <= 127; k++) rhos.push_back(jp_mip_from_bits((unsigned int)(127 + k) << 23));
	for (float r : rhos)
	{   // the level is the exponent, the fraction lies in [0, 1)
		const int l = jp_mip_level_of(r);
		if (l < 0 || l > 127) bad++;
		if (l < JP_MIP_MAX_LEVELS) { const float f = jp_mip_fraction(r, l); if (!(f >= 0.f && f < 1.f)) bad++; }
	}
	for (const auto& sz : sizes)
	{
		const int w = sz[0], h = sz[1];
		std::vector<JpMipLevel> lev; std::vector<unsigned int*> blocks;
		int lw = w, lh = h;
		for (int k = 0; k < jp_mip_levels(w, h); k++)
		{   // one heap block per level, exactly its texels: the sanitizer sees any tap outside it
			unsigned int* p = (unsigned int*)malloc((size_t)lw * lh * sizeof(unsigned int));
			if (k == 0) for (size_t i = 0; i < (size_t)lw * lh; i++) p[i] = (unsigned int)((i * 2654435761u) >> 8) | 0xff000000u;
			else for (int j = 0; j < lh; j++) for (int i = 0; i < lw; i++) p[(size_t)j * lw + i] = jp_mip_down_texel(blocks[k - 1], lev[k - 1].w, lev[k - 1].h, i, j);
			const JpMipLevel l = { lw, lh, 0, 0 }; lev.push_back(l); blocks.push_back(p);
			lw = jp_mip_half(lw); lh = jp_mip_half(lh);
		}
		if (lev.back().w != 1 || lev.back().h != 1 || (int)lev.size() > JP_MIP_MAX_LEVELS) bad++;
		// the lookup reads a level at texels + first: one contiguous chain, again of exactly its texels
		size_t chain = 0; for (const JpMipLevel& l : lev) chain += (size_t)l.w * l.h;
		unsigned int* texels = (unsigned int*)malloc(chain * sizeof(unsigned int));
		size_t at = 0;
		for (size_t k = 0; k < lev.size(); k++) { lev[k].first = (int32_t)at; for (size_t i = 0; i < (size_t)lev[k].w * lev[k].h; i++) texels[at + i] = blocks[k][i]; at += (size_t)lev[k].w * lev[k].h; }
		std::vector<float> e = { 0.f, -0.f, 1.f, -1e-10f, 1.f - 5.9604645e-8f, 16777216.f, -16777216.f, 3e38f, -3e38f, inf, -inf, nan, 0.99999994f, 1.0000001f, -1.f, 2.f, -3.f, 0.5f };
		for (int size : { w, h }) if (size <= 64) for (int k = -size; k <= 2 * size; k += (size > 8 ? 7 : 1)) e.push_back((float)k / (float)size);
		long long n = 0;
		for (int wu = 0; wu < 3; wu++) for (int wv = 0; wv < 3; wv++)
			for (float sc : { 1.f, 3.f, 3e38f, 1e-38f })
			{
				const JpTexSampler s = { wu, wv, JP_FILTER_BILINEAR, sc, 2.f, sc > 1.f ? -0.3f : 0.f, 100.125f };
				for (float r : rhos) for (float u : e) for (float v : e) { if (jp_mip_lookup_above(&s, texels, lev.data(), (int)lev.size(), u, v, r) > 0xffffffu) bad++; n++; }
			}
		printf("%5d x %-5d %zu levels, %lld lookups on %zu coordinates per axis and %zu footprints\n", w, h, lev.size(), n, e.size(), rhos.size());
		total += n;
		for (unsigned int* p : blocks) free(p);
		free(texels);
	}
	// the footprint: 0 wherever it is not a finite number of texels
	const float widths[] = { 0.f, 1.f, 3e38f, inf, nan, -1.f, 1e-45f }, areas[] = { 0.f, -1.f, 1.f, 1e-45f, 3e38f, inf, nan };
	for (float wd : widths) for (float a : areas) for (float sc : { 1.f, 3e38f, 1e-38f })
	{
		const float r = jp_mip_rho(wd, a, 16384, 16384, sc, sc, 1.f);
		if (!(r - r == 0.f)) bad++;
		if (!(a > 0.f) || !(a - a == 0.f)) { if (r != 0.f) bad++; }
		total++;
	}
	const float tri[3][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 } }, uv_same[6] = { 0.3f, 0.3f, 0.3f, 0.3f, 0.3f, 0.3f }, uv_nan[6] = { 0, 0, nan, 0, 0, 1 }, uv_ok[6] = { 0, 0, 2, 0, 0, 2 };
	if (jp_mip_area_triangle(tri[0], tri[1], tri[2], uv_same) != 0.f || jp_mip_area_triangle(tri[0], tri[1], tri[2], uv_nan) != 0.f) bad++;
	if (jp_mip_area_triangle(tri[0], tri[1], tri[2], uv_ok) != 0.25f) bad++;
	const float zero[3] = { 0, 0, 0 };
	if (jp_mip_area_sphere(zero, 2.f) != 0.f || jp_mip_area_disk(zero, 2.f) != 0.f) bad++;
	// the cone: bounce 0 overwrites whatever the slot held; a specular bounce keeps the spread, any other raises it to bounce_spread at least
	for (float w0 : widths) for (float s0 : widths)
	{
		float wd = w0, sp = s0;
		jp_mip_cone_hit(0.01f, 0.125f, 0 | (7 << 16), 10.f, &wd, &sp);
		if (sp != 0.01f || wd != 0.01f * 10.f) bad++;
		jp_mip_cone_hit(0.01f, 0.125f, 1 | 0x100, 5.f, &wd, &sp);
		if (sp != 0.01f) bad++;
		jp_mip_cone_hit(0.01f, 0.125f, 2, 5.f, &wd, &sp);
		if (sp != 0.125f) bad++;
		sp = s0; wd = w0;
		jp_mip_cone_hit(0.01f, 0.125f, 3, 5.f, &wd, &sp);
		if (!(sp >= 0.125f)) bad++;                                        // (a NaN spread becomes bounce_spread)
		total += 4;
	}
	printf("%lld checks, %d failed\n", total, bad);
	return bad ? 1 : 0;
}
