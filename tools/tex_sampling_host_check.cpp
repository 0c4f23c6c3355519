// tools/tex_sampling_host_check.cpp -- include/jp_tex_sampling.h as a stand-alone program for AddressSanitizer / UBSan: every wrap_u x wrap_v x filter on the edge
// set of coordinates (+-0, 1, integers, texel boundaries, -1e-10, 1 - 2^-24, +-2^24, +-3e38, +-inf, NaN) times the scales and offsets of the host test, on images
// whose texel arrays are heap blocks of exactly w * h dwords: a tap outside the image, a float-to-int cast of a value outside the int range or of a NaN, or a signed
// overflow ends the program.  The colour lookup, the normal-map lookup and the lookup without records.  No context, no device: nothing is loaded into Python and
// nothing runs on a GPU.  From the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -Iinclude tools/tex_sampling_host_check.cpp -o tex_sampling_host_check
//   ./tex_sampling_host_check        (prints one line per image size, exit status 0 when every lookup stayed inside its image and delivered a defined value)
#include "jp_tex_sampling.h"
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

int main()
{
	const int sizes[][2] = { { 1, 1 }, { 1, 7 }, { 5, 3 }, { 8, 8 }, { 16384, 1 } };
	const float scales[] = { 0.5f, 1.f, 2.f, 3.f, 7.25f, 3e38f, 1e-38f }, offsets[] = { 0.f, 0.5f, -0.3f, 100.125f, -3e38f };
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	long long total = 0; int bad = 0;
	for (const auto& sz : sizes)
	{
		const int w = sz[0], h = sz[1];
		unsigned int* texels = (unsigned int*)malloc((size_t)w * h * sizeof(unsigned int));      // exactly the image: the sanitizer sees any tap outside it
		for (size_t k = 0; k < (size_t)w * h; k++) texels[k] = (unsigned int)((k * 2654435761u) >> 8) | 0xff000000u;
		std::vector<float> e = { 0.f, -0.f, 1.f, -1e-10f, 1.f - 5.9604645e-8f, 16777216.f, -16777216.f, 3e38f, -3e38f, inf, -inf, nan, 0.99999994f, 1.0000001f, -1.f, 2.f, 3.f, -2.f, -3.f, 4.f };
		for (int size : { w, h }) if (size <= 64) for (int k = -size; k <= 2 * size; k++) e.push_back((float)k / (float)size);
		long long n = 0;
		for (int wu = 0; wu < 3; wu++) for (int wv = 0; wv < 3; wv++) for (int f = 0; f < 3; f++)
			for (float su : scales) for (float ou : offsets)
			{
				const JpTexSampler s = { wu, wv, f, su, scales[(int)(ou != 0.f)], ou, offsets[(int)(su > 1.f)] };
				const bool nmap_ok = wu != JP_WRAP_MIRROR && wv != JP_WRAP_MIRROR && f != JP_FILTER_NEAREST;
				for (float u : e) for (float v : e)
				{
					const unsigned int c = jp_tex_lookup_sampled(&s, texels, w, h, u, v);
					if (c > 0xffffffu) bad++;
					if (nmap_ok)
					{
						float m[3]; jp_nmap_lookup_sampled(&s, texels, w, h, u, v, m);
						for (int k = 0; k < 3; k++) if (!(m[k] >= -1.001f && m[k] <= 1.001f)) bad++;      // (between its four taps up to rounding)
					}
					n++;
				}
			}
		for (float u : e) for (float v : e) { if (jp_tsamp_nearest_clamp(w, h, u, v) >= (size_t)w * h) bad++; n++; }
		printf("%5d x %-5d %lld lookups on %zu coordinates per axis\n", w, h, n, e.size());
		total += n;
		free(texels);
	}
	printf("%lld lookups, %d outside their range\n", total, bad);
	return bad ? 1 : 0;
}
