// tools/variance_host_check.cpp -- include/jp_variance.h as a stand-alone program for AddressSanitizer / UBSan: jp_var_samples, the body of jp_variance_samples, on
// heap blocks of exactly its samples and outputs (a read or write outside them ends the program), over edge inputs: spp 2 .. 257, constant pixels (variance exactly
// 0), one sample of 1e6, samples of 3e38, infinities, NaNs and negative zeros in any channel, with the sample clamp off and on (tiny, 1, huge), either output null,
// no pixels at all.  No context, no device: nothing is loaded into Python and nothing runs on a GPU.  From the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/variance_host_check.cpp -o variance_host_check
//   ./variance_host_check        (prints one line per sample count, exit status 0 when every variance of finite samples was finite and >= 0 and every constant pixel gave 0)
#include "jp_variance.h"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

int main()
{
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const float edge[] = { 0.f, -0.f, 1.f, 0.1f, 1e-45f, 1e-38f, 1e6f, 3e38f, 3.4028235e38f, inf, -inf, nan, -1.f };
	const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
	const float clamps[] = { 0.f, 1e-30f, 1.f, 3e38f };
	long long total = 0; int bad = 0;
	for (int spp : { 2, 3, 16, 257 })
	{
		// pixels: [0, n_edge) constant at an edge value; [n_edge, 2 n_edge) 0.5 with one edge sample in the middle; then n_edge^2 pixels with an edge value in two
		// channels of the last sample; the rest pseudo-random
		const long long n = 2 * n_edge + (long long)n_edge * n_edge + 37;
		float* s = (float*)malloc((size_t)spp * n * 3 * sizeof(float));
		float* var = (float*)malloc((size_t)n * sizeof(float));
		float* mean = (float*)malloc((size_t)n * sizeof(float));
		unsigned int h = 12345u;
		for (int k = 0; k < spp; k++) for (long long p = 0; p < n; p++) for (int c = 0; c < 3; c++)
		{
			h = h * 1664525u + 1013904223u;
			float v = (float)(h >> 8) * (1.0f / 16777216.0f);
			if (p < n_edge) v = edge[p];
			else if (p < 2 * n_edge) v = k == spp / 2 ? edge[p - n_edge] : 0.5f;
			else if (p < 2 * n_edge + (long long)n_edge * n_edge && k == spp - 1 && c < 2) v = c == 0 ? edge[(p - 2 * n_edge) / n_edge] : edge[(p - 2 * n_edge) % n_edge];
			s[3 * ((size_t)k * n + p) + c] = v;
		}
		for (float cl : clamps)
		{
			jp_var_samples(cl, spp, n, s, var, mean);
			for (long long p = 0; p < n; p++)
			{
				total++;
				const bool finite_in = p >= 2 * n_edge + (long long)n_edge * n_edge || (p < n_edge && edge[p] - edge[p] == 0.f && (edge[p] < 1e30f && edge[p] > -1e30f));
				if (p < n_edge && (edge[p] - edge[p] == 0.f) && edge[p] < 1e30f && var[p] != 0.f) bad++;      // a constant pixel: exactly 0
				if (p < n_edge && !(edge[p] - edge[p] == 0.f) && (var[p] != 0.f || mean[p] != 0.f)) bad++;     // not finite: every sample counts as 0
				if (finite_in && !(var[p] >= 0.f && var[p] - var[p] == 0.f)) bad++;
			}
			// either output may be null, and no pixels is no access
			float v1 = -1.f, m1 = -1.f;
			jp_var_samples(cl, spp, 1, s, &v1, nullptr); jp_var_samples(cl, spp, 1, s, nullptr, &m1);
			if (v1 == -1.f || m1 == -1.f) bad++;                              // (the block read as [spp][1][3]: its first spp triples; both outputs written)
			jp_var_samples(cl, spp, 0, nullptr, nullptr, nullptr);
			total += 3;
		}
		printf("spp %3d: %lld pixels x %d clamps\n", spp, n, (int)(sizeof(clamps) / sizeof(clamps[0])));
		free(s); free(var); free(mean);
	}
	// the steps themselves: Welford on two samples, the variance of the mean of two
	{
		float mean = 0.f, m2 = 0.f;
		jp_var_step(&mean, &m2, 1.f, 1); jp_var_step(&mean, &m2, 3.f, 2);
		if (mean != 2.f || m2 != 2.f || jp_var_of_mean(m2, 2) != 1.f) bad++;
		if (jp_var_luminance(nan, 0.f, 0.f) != 0.f || jp_var_luminance(inf, 0.f, 0.f) != 0.f || jp_var_luminance(0.f, 3.4e38f, 3.4e38f * 16.f) != 0.f) bad++;
		total += 2;
	}
	printf("%lld checks, %d failed\n", total, bad);
	return bad ? 1 : 0;
}
