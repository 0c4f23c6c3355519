// tools/adaptive_host_check.cpp -- include/jp_adaptive.h as a stand-alone program for AddressSanitizer / UBSan: jp_adapt_samples, the body of jp_adaptive_samples, on
// heap blocks of exactly its samples, scratch and outputs (a read or write outside them ends the program), over edge inputs: images of 1 x 1, 1 x 7, 7 x 1, 40 x 24 and
// 5 x 9 pixels, whole and as band shards (bands of 1, 2, 4 rows dealt to 1 .. 3 shards: the clipped neighbourhood, the row maps), both dilate values, min = max,
// a step larger than what is left, thresholds 0 and huge, the sample clamp off and on, hdr 0 / 1, every output null in turn, and samples that are constant, alternate,
// overflow the moments (3e38), or hold infinities and NaNs.  It checks what must hold whatever the samples are: counts are min + k * step or max, 0 outside the
// shard; with dilate = 0 the shards' planes add up to the whole image's bit for bit; dilate = 1 never gives a pixel fewer samples than dilate = 0; the film is
// never negative or NaN.  No context, no device: nothing is loaded into Python and nothing runs on a GPU.  From the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/adaptive_host_check.cpp -o adaptive_host_check
//   ./adaptive_host_check        (prints one line per image size, exit status 0 when every check held)
#include "jp_adaptive.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

struct Planes { float* film; int32_t* counts; float* var; };
static Planes planes(size_t n) { Planes p = { (float*)malloc(3 * n * sizeof(float)), (int32_t*)malloc(n * sizeof(int32_t)), (float*)malloc(n * sizeof(float)) }; return p; }
static void drop(Planes p) { free(p.film); free(p.counts); free(p.var); }

int main()
{
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const float edge[] = { 0.f, -0.f, 1.f, 0.1f, 1e-45f, 1e6f, 3e38f, inf, -inf, nan, -1.f };
	const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
	const int sizes[][2] = { { 1, 1 }, { 7, 1 }, { 1, 7 }, { 40, 24 }, { 5, 9 } };              // (width, height)
	const int spp_sets[][3] = { { 2, 1, 2 }, { 2, 1, 5 }, { 4, 4, 14 }, { 3, 100, 9 }, { 8, 8, 32 } };   // (min, step, max)
	int bad = 0; long long runs = 0;
	for (const auto& wh : sizes)
	{
		const int W = wh[0], H = wh[1]; const size_t n = (size_t)W * H;
		for (const auto& sp : spp_sets)
		{
			const int mn = sp[0], step = sp[1], mx = sp[2];
			// the whole image's samples [mx][n][3]: pixel p < n_edge constant at an edge value, the next n_edge 0.5 with one edge sample, then alternating pixels, then pseudo-random ones
			float* s = (float*)malloc((size_t)mx * n * 3 * sizeof(float));
			unsigned int h = 777u;
			for (int k = 0; k < mx; k++) for (size_t p = 0; p < n; p++) for (int c = 0; c < 3; c++)
			{
				h = h * 1664525u + 1013904223u;
				float v = (float)(h >> 8) * (1.0f / 16777216.0f);
				if (p < (size_t)n_edge) v = edge[p];
				else if (p < 2 * (size_t)n_edge) v = k == mx / 2 ? edge[p - n_edge] : 0.5f;
				else if (p % 3 == 0) v = (k & 1) ? 2.5f : 0.25f;
				else if (p % 3 == 1) v = 0.375f;
				s[3 * ((size_t)k * n + p) + c] = v;
			}
			for (float thr : { 0.f, 0.05f, 3e38f }) for (float cl : { 0.f, 1.f }) for (int hdr = 0; hdr < 2; hdr++)
			{
				Planes whole[2] = { planes(n), planes(n) };
				for (int dilate = 0; dilate < 2; dilate++)
				{
					JpAdaptive a = { (int32_t)sizeof(JpAdaptive), mn, step, mx, thr, 0.f, dilate };
					if (jp_adapt_check(&a) != 0) { bad++; continue; }
					const JpAdaptShard sh = { W, H, H, 0, 1 };
					float* scratch = (float*)malloc((size_t)jp_adapt_scratch_floats((int64_t)n) * sizeof(float));
					jp_adapt_samples(cl, hdr, &a, &sh, s, scratch, whole[dilate].film, whole[dilate].counts, whole[dilate].var); runs++;
					jp_adapt_samples(cl, hdr, &a, &sh, s, scratch, nullptr, whole[dilate].counts, nullptr);            // null outputs
					jp_adapt_samples(cl, hdr, &a, &sh, s, scratch, whole[dilate].film, nullptr, whole[dilate].var);
					free(scratch);
					for (size_t p = 0; p < n; p++)
					{
						const int c = whole[dilate].counts[p];
						if (!(c == mx || (c >= mn && c < mx && (c - mn) % step == 0))) bad++;
						for (int k = 0; k < 3; k++) { const float v = whole[dilate].film[3 * p + k]; if (!(v >= 0.f) || (!hdr && v > 1.f)) bad++; }
						if (thr == 0.f && dilate == 0 && c != mx && whole[dilate].var[p] != 0.f && jp_film_finite(whole[dilate].var[p])) bad++;   // threshold 0 stops only a pixel whose samples were all equal (or whose moments overflowed)
					}
					// band shards: each shard gets its own samples [mx][local pixels][3], cut from the whole image's
					for (int band : { 1, 2, 4 }) for (int count = 1; count <= 3; count++)
					{
						Planes sum = planes(n);
						memset(sum.film, 0, 3 * n * sizeof(float)); memset(sum.counts, 0, n * sizeof(int32_t)); memset(sum.var, 0, n * sizeof(float));
						for (int index = 0; index < count; index++)
						{
							const JpAdaptShard ss = { W, H, band, index, count };
							const int rows = jp_adapt_local_rows(&ss); const size_t np = (size_t)rows * W;
							float* ls = (float*)malloc((np ? (size_t)mx * np * 3 : 1) * sizeof(float));
							for (int r = 0; r < rows; r++)
							{
								const int y = jp_adapt_film_row(&ss, r);
								if (y < 0 || y >= H || jp_adapt_local_row(&ss, y) != r) { bad++; continue; }
								for (int k = 0; k < mx; k++) memcpy(ls + 3 * ((size_t)k * np + (size_t)r * W), s + 3 * ((size_t)k * n + (size_t)y * W), 3 * (size_t)W * sizeof(float));
							}
							Planes part = planes(n);
							float* sc = (float*)malloc(((size_t)jp_adapt_scratch_floats((int64_t)np) + 1) * sizeof(float));
							jp_adapt_samples(cl, hdr, &a, &ss, ls, sc, part.film, part.counts, part.var); runs++;
							for (size_t p = 0; p < n; p++)
							{
								const bool mine = jp_adapt_local_row(&ss, (int)(p / W)) >= 0;
								if (!mine && (part.counts[p] != 0 || part.var[p] != 0.f)) bad++;
								if (mine && dilate == 1 && part.counts[p] > whole[1].counts[p]) bad++;                    // a clipped neighbourhood holds fewer failing pixels, never more
								sum.counts[p] += part.counts[p]; sum.var[p] += part.var[p];
								for (int k = 0; k < 3; k++) sum.film[3 * p + k] += part.film[3 * p + k];
							}
							free(sc); free(ls); drop(part);
						}
						if (dilate == 0 && (memcmp(sum.counts, whole[0].counts, n * sizeof(int32_t)) || memcmp(sum.var, whole[0].var, n * sizeof(float)) || memcmp(sum.film, whole[0].film, 3 * n * sizeof(float)))) bad++;
						drop(sum);
					}
				}
				for (size_t p = 0; p < n; p++) if (whole[1].counts[p] < whole[0].counts[p]) bad++;
				drop(whole[0]); drop(whole[1]);
			}
			free(s);
		}
		printf("%d x %d: %lld runs so far, %d checks failed\n", W, H, runs, bad);
	}
	// the argument checks
	JpAdaptive ok = { (int32_t)sizeof(JpAdaptive), 8, 8, 32, 0.05f, 0.f, 1 };
	JpAdaptive b;
	if (jp_adapt_check(&ok) != 0) bad++;
	b = ok; b.min_spp = 1; if (jp_adapt_check(&b) != 2) bad++;
	b = ok; b.step_spp = 0; if (jp_adapt_check(&b) != 3) bad++;
	b = ok; b.max_spp = 7; if (jp_adapt_check(&b) != 4) bad++;
	b = ok; b.max_spp = 0; if (jp_adapt_check(&b) != 0) bad++;
	b = ok; b.threshold = nan; if (jp_adapt_check(&b) != 5) bad++;
	b = ok; b.threshold = -1.f; if (jp_adapt_check(&b) != 5) bad++;
	b = ok; b.floor = inf; if (jp_adapt_check(&b) != 6) bad++;
	b = ok; b.dilate = 2; if (jp_adapt_check(&b) != 7) bad++;
	b = ok; b.struct_bytes = 4; if (jp_adapt_check(&b) != 1) bad++;
	printf("%s\n", bad ? "FAILED" : "ok");
	return bad ? 1 : 0;
}
