// tools/procedural_host_check.cpp -- include/jp_procedural.h as a stand-alone program for AddressSanitizer / UBSan: every kind, both spaces, the identity and a
// general map, antialias on and off, over the product of a hostile coordinate set (NaN, +-infinity, +-2^24 and its neighbours, +-FLT_MAX, denormals, negative
// lattice cells, lattice points) with a hostile width set (NaN, infinity, negative, denormal, the fade boundaries, huge).  A float-to-int conversion outside the
// integer's range ends the program (-fsanitize=float-cast-overflow); beyond that it checks what the header promises: t in [0, 1], a tagged word, |n| <= 1, n = 0 on
// the lattice and outside the range.  No context, no device: nothing is loaded into Python and nothing runs on a GPU.  From the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -Iinclude tools/procedural_host_check.cpp -o procedural_host_check
//   ./procedural_host_check    (prints one line per kind, exit status 0 when every value was defined and every promise held)
#include "jp_procedural.h"
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

int main()
{
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), big = 16777216.f;
	const std::vector<float> xs = { 0.f, -0.f, 1.f, -1.f, 0.5f, -0.5f, -3.f, -2.75f, 7.25f, 1e-45f, -1e-45f, 1e-39f, FLT_MIN, big, -big, nextafterf(big, 0.f), -nextafterf(big, 0.f), big * 2.f,
	                                big / 2.f + 0.5f, -big / 2.f - 0.5f, big / 4096.f, 1e30f, -1e30f, FLT_MAX, -FLT_MAX, inf, -inf, nan, 0.31415927f, 1.5707964f, 123456.79f, -65535.996f };
	std::vector<float> ws = { 0.f, -0.f, -1.f, nan, inf, -inf, 1e-45f, FLT_MIN, 1e-30f, 0.01f, 0.1f, 0.3f, 1.f, 100.f, 5000.f, 1e30f, FLT_MAX };
	for (int o = 0; o < JP_PROC_MAX_OCTAVES; o++)
		for (float k : { 0.25f, 0.5f }) { const float x = k / (float)(1 << o); ws.push_back(x); ws.push_back(nextafterf(x, 0.f)); ws.push_back(nextafterf(x, 1.f)); }
	const float maps[2][12] = { { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 }, { 2.f, 0.5f, 0.f, 0.25f, -0.5f, 1.5f, 0.25f, -1.f, 0.f, 0.25f, 3e18f, 0.5f } };
	const float ce[3] = { 0.125f, 0.5f, 0.875f }, co[3] = { 1.f, 0.25f, 0.f };
	long long total = 0; int bad = 0;
	// the noise by itself
	for (float x : xs) for (float y : xs) for (float z : xs)
	{
		const float n = jp_proc_noise(x, y, z);
		total++;
		if (!(n >= -1.f && n <= 1.f)) bad++;
		const bool in = jp_proc_in_range(x) && jp_proc_in_range(y) && jp_proc_in_range(z);
		if ((!in || (x == floorf(x) && y == floorf(y) && z == floorf(z))) && n != 0.f) bad++;
	}
	printf("noise: %lld points, %d broken promises\n", total, bad);
	for (int kind = JP_PROC_NOISE; kind <= JP_PROC_CHECKER_AA; kind++)
	{
		long long count = 0; int before = bad;
		for (int space = 0; space < 2; space++) for (int m = 0; m < 2; m++) for (int aa = -1; aa <= 1; aa++) for (int oct : { 0, 1, 12 })
		{
			JpProcedural r; std::memset(&r, 0, sizeof(r));
			r.kind = kind; r.space = space; std::memcpy(r.m, maps[m], sizeof(r.m)); r.octaves = oct; r.gain = oct == 12 ? 1.f : 0.f; r.variation = m ? 1e20f : 0.f; r.antialias = aa;
			if (jp_procedural_check(&r)) { bad++; continue; }
			const JpProcDev d = jp_proc_resolve(&r);
			for (float x : xs) for (float y : xs) for (float z : { xs[0], xs[5], xs[13], xs[23], xs[25], xs[27], xs[30] }) for (float w : ws)
			{
				const float p[3] = { x, y, z };
				float t = -1.f;
				const unsigned int word = jp_proc_lookup(&d, ce, co, 1234567, p, y, x, w, &t);
				count++;
				if (!(t >= 0.f && t <= 1.f)) bad++;
				if (word & JP_PROC_TAG_IMAGE) { if (word & 0x7f000000u) bad++; }
				else if (kind != JP_PROC_CHECKER_AA || (word & ~1u) != (JP_PROC_TAG_COLOR | (2u * 1234567u))) bad++;
			}
		}
		total += count;
		printf("kind %d: %lld lookups, %d broken promises\n", kind, count, bad - before);
	}
	// the checks of a record: every rule fires on its own field and on nothing else
	{
		JpProcedural r; std::memset(&r, 0, sizeof(r));
		r.kind = JP_PROC_FBM; std::memcpy(r.m, maps[0], sizeof(r.m));
		if (jp_procedural_check(&r) != 0) bad++;
		JpProcedural q = r; q.kind = 9; if (jp_procedural_check(&q) != 1) bad++;
		q = r; q.space = -1; if (jp_procedural_check(&q) != 2) bad++;
		q = r; q.m[7] = nan; if (jp_procedural_check(&q) != 3) bad++;
		q = r; q.m[0] = 0.f; if (jp_procedural_check(&q) != 4) bad++;
		q = r; q.m[0] = q.m[5] = q.m[10] = FLT_MAX; if (jp_procedural_check(&q) != 4) bad++;
		q = r; q.octaves = 13; if (jp_procedural_check(&q) != 5) bad++;
		q = r; q.gain = 1.0000001f; if (jp_procedural_check(&q) != 6) bad++;
		q = r; q.variation = inf; if (jp_procedural_check(&q) != 7) bad++;
		q = r; q.antialias = -2; if (jp_procedural_check(&q) != 8) bad++;
	}
	printf("%lld evaluations, %d broken promises\n", total, bad);
	return bad ? 1 : 0;
}
