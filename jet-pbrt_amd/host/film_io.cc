// jet-pbrt_amd/host/film_io.cc -- FFilm::SaveAsImage (film.h:84, film.cc:11-188): the step right after the hot path
// (main.cc:160).  Own writers for the three formats the reference offers; same file names (<name>.ppm/.bmp/.hdr),
// same tone curve for the 8-bit formats (gamma_encoding, film.h:24), top row first in the film, and the format
// rules applied properly where the reference's writers are off:
//   * PPM "P3" samples are written as decimal numbers (the reference streams uint8_t, i.e. raw characters);
//   * BMP rows are padded to 4 bytes and the padded rows are what gets written (the reference computes the padded
//     layout but writes width*3-byte rows, so widths with width*3 % 4 != 0 come out sheared);
//   * HDR pixels below 1e-32 are written as zero RGBE (the reference leaves them uninitialised).
#include "jetpbrt.h"

#include <algorithm>
#include <cstring>
#include <cctype>
#include <fstream>
#include <iostream>
#include <iterator>
#include <atomic>

namespace jetpbrt
{
namespace
{
// 8-bit pixels of the film: the device-encoded bytes when the integrator delivered them (FFilm::RequestDeviceLDR), else
// gamma_encoding (film.h:24) of the fp32 pixels on the host -- the two are byte-identical (tests)
std::vector<uint8_t> Pixels8(int w, int h, const std::vector<FColor>& px, const std::vector<uint8_t>& ldr8)
{
	if (ldr8.size() == (size_t)w * h * 3) return ldr8;
	std::vector<uint8_t> b((size_t)w * h * 3);
	for (size_t i = 0; i < px.size(); i++) { b[3 * i] = gamma_encoding(px[i].r); b[3 * i + 1] = gamma_encoding(px[i].g); b[3 * i + 2] = gamma_encoding(px[i].b); }
	return b;
}

bool WritePPM(const std::string& path, int w, int h, const std::vector<uint8_t>& p8)
{
	std::ofstream f(path, std::ios::binary | std::ios::out);
	if (!f.is_open()) return false;
	f << "P3\n" << w << " " << h << "\n255\n";
	for (size_t i = 0; i < (size_t)w * h; i++)
		f << (int)p8[3 * i] << "  " << (int)p8[3 * i + 1] << "  " << (int)p8[3 * i + 2] << "\n";
	return (bool)f;
}

void put16(std::vector<uint8_t>& b, size_t at, uint16_t v) { b[at] = (uint8_t)v; b[at + 1] = (uint8_t)(v >> 8); }
void put32(std::vector<uint8_t>& b, size_t at, uint32_t v) { for (int k = 0; k < 4; k++) b[at + k] = (uint8_t)(v >> (8 * k)); }

bool WriteBMP(const std::string& path, int w, int h, const std::vector<uint8_t>& p8)
{
	const size_t row = ((size_t)w * 3 + 3) & ~(size_t)3, body = row * h, head = 14 + 40;
	std::vector<uint8_t> b(head + body, 0);
	b[0] = 'B'; b[1] = 'M';
	put32(b, 2, (uint32_t)(head + body)); put32(b, 10, (uint32_t)head);
	put32(b, 14, 40); put32(b, 18, (uint32_t)w); put32(b, 22, (uint32_t)h); put16(b, 26, 1); put16(b, 28, 24);
	// biSizeImage stays 0, as the reference writes it (legal for BI_RGB): for widths whose rows need no padding the file is then
	// byte-identical to the reference's (tests/golden/film_io.npz)
	for (int y = 0; y < h; y++)                                  // BMP stores the bottom row first
	{
		uint8_t* line = &b[head + row * (size_t)(h - 1 - y)];
		for (int x = 0; x < w; x++)
		{
			const uint8_t* c = &p8[3 * ((size_t)y * w + x)];
			line[3 * x + 0] = c[2]; line[3 * x + 1] = c[1]; line[3 * x + 2] = c[0];                   // B G R
		}
	}
	std::ofstream f(path, std::ios::binary | std::ios::out);
	if (!f.is_open()) return false;
	f.write((const char*)b.data(), (std::streamsize)b.size());
	return (bool)f;
}

bool WriteHDR(const std::string& path, int w, int h, const std::vector<FColor>& px)
{
	std::ofstream f(path, std::ios::binary | std::ios::out);
	if (!f.is_open()) return false;
	f << "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y " << h << " +X " << w << "\n";
	for (size_t i = 0; i < px.size(); i++)
	{
		uint8_t rgbe[4] = { 0, 0, 0, 0 };
		const FColor& c = px[i];
		const float v = std::max(c.r, std::max(c.g, c.b));
		if (v >= 1e-32f)
		{
			int e; const float m = (float)(std::frexp(v, &e) * 256.f / v);   // v = mantissa * 2^e; channel byte = channel * 256 * mantissa / v
			rgbe[0] = (uint8_t)(c.r * m); rgbe[1] = (uint8_t)(c.g * m); rgbe[2] = (uint8_t)(c.b * m); rgbe[3] = (uint8_t)(e + 128);
		}
		f.write((const char*)rgbe, 4);
	}
	return (bool)f;
}
}

bool FFilm::SaveAsImage(const std::string& filename, EImageType imgType) const
{
	switch (imgType)
	{
	case EImageType::PPM: return WritePPM(filename + ".ppm", width, height, Pixels8(width, height, pixels, ldr8));
	case EImageType::BMP: return WriteBMP(filename + ".bmp", width, height, Pixels8(width, height, pixels, ldr8));
	case EImageType::HDR: return floatValid ? WriteHDR(filename + ".hdr", width, height, pixels) : false;   // an LDR-only render left no fp32 pixels to write
	}
	return false;
}

} // namespace jetpbrt

// ---- image readers of FImageTexture (texture.cc reads with stb_image; here: the two formats this library writes) ---------------
namespace jetpbrt
{
namespace
{
// PPM header token: skips whitespace and '#' comments
bool PpmToken(const std::vector<uint8_t>& f, size_t& at, long& v)
{
	for (;;)
	{
		while (at < f.size() && std::isspace(f[at])) at++;
		if (at < f.size() && f[at] == '#') { while (at < f.size() && f[at] != '\n') at++; continue; }
		break;
	}
	if (at >= f.size() || !std::isdigit(f[at])) return false;
	v = 0;
	while (at < f.size() && std::isdigit(f[at])) { v = v * 10 + (f[at] - '0'); if (v > (1l << 30)) return false; at++; }
	return true;
}
uint32_t Get32(const std::vector<uint8_t>& b, size_t at) { return (uint32_t)b[at] | ((uint32_t)b[at + 1] << 8) | ((uint32_t)b[at + 2] << 16) | ((uint32_t)b[at + 3] << 24); }
uint16_t Get16(const std::vector<uint8_t>& b, size_t at) { return (uint16_t)(b[at] | (b[at + 1] << 8)); }
}

bool ReadImageRGB8(const char* filename, std::vector<uint8_t>& rgb, int& width, int& height)
{
	rgb.clear(); width = height = 0;
	if (!filename) return false;
	std::ifstream in(filename, std::ios::binary);
	if (!in) return false;
	std::vector<uint8_t> f((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	if (f.size() >= 2 && f[0] == 'P' && f[1] == '6')
	{   // binary PPM, maxval 255: one whitespace byte after the maxval, then rows top first
		size_t at = 2; long w = 0, h = 0, mx = 0;
		if (!PpmToken(f, at, w) || !PpmToken(f, at, h) || !PpmToken(f, at, mx)) return false;
		if (mx != 255 || w < 1 || h < 1 || w > 16384 || h > 16384 || at >= f.size() || !std::isspace(f[at])) return false;
		at++;
		const size_t n = (size_t)w * h * 3;
		if (f.size() - at < n) return false;
		rgb.assign(f.begin() + at, f.begin() + at + n);
		width = (int)w; height = (int)h;
		return true;
	}
	if (f.size() >= 54 && f[0] == 'B' && f[1] == 'M')
	{   // uncompressed 24 / 32-bit BMP: BGR(A) rows padded to 4 bytes, bottom-up (a negative height: top-down)
		const uint32_t off = Get32(f, 10), hdr = Get32(f, 14);
		if (hdr < 40) return false;
		const int32_t w = (int32_t)Get32(f, 18), hs = (int32_t)Get32(f, 22);
		const uint16_t planes = Get16(f, 26), bpp = Get16(f, 28);
		const uint32_t comp = Get32(f, 30);
		if (planes != 1 || (bpp != 24 && bpp != 32) || !(comp == 0 || (comp == 3 && bpp == 32))) return false;
		// channel positions in a little-endian pixel: B G R (X) unless BI_BITFIELDS masks say otherwise; a mask must select one whole byte
		int shift[3] = { 16, 8, 0 };                                  // R, G, B
		if (comp == 3)
		{   // the masks follow a 40-byte header, and sit at the same place inside a V4 / V5 header
			if (f.size() < 66) return false;
			for (int k = 0; k < 3; k++)
			{
				const uint32_t m = Get32(f, 54 + 4 * k);
				int sh = -1;
				for (int b = 0; b < 4; b++) if (m == (0xffu << (8 * b))) sh = 8 * b;
				if (sh < 0) return false;
				shift[k] = sh;
			}
			if (shift[0] == shift[1] || shift[0] == shift[2] || shift[1] == shift[2]) return false;
		}
		const long long h = hs < 0 ? -(long long)hs : hs;
		if (w < 1 || h < 1 || w > 16384 || h > 16384) return false;
		const size_t bytes = bpp / 8, row = ((size_t)w * bytes + 3) & ~(size_t)3;
		if (off > f.size() || f.size() - off < row * (size_t)h) return false;
		rgb.resize((size_t)w * h * 3);
		for (long long y = 0; y < h; y++)
		{
			const size_t src = off + row * (size_t)(hs < 0 ? y : h - 1 - y);
			for (int x = 0; x < w; x++)
			{
				uint8_t* o = &rgb[3 * ((size_t)y * w + x)];
				const uint8_t* p = &f[src + bytes * x];
				for (int k = 0; k < 3; k++) o[k] = p[shift[k] / 8];
			}
		}
		width = w; height = (int)h;
		return true;
	}
	return false;
}

FImageTexture::FImageTexture(const char* filename) : width(0), height(0)
{
	if (!ReadImageRGB8(filename, data, width, height))
	{
		std::cerr << "ERROR: Could not load texture image file" << (filename ? filename : "") << ".\n";   // texture.cc (the reference's message)
		data.clear(); width = height = 0;
	}
}

FImageTexture::FImageTexture(const uint8_t* rgb8, int w, int h) : width(0), height(0)
{
	if (rgb8 && w > 0 && h > 0) { data.assign(rgb8, rgb8 + (size_t)w * h * 3); width = w; height = h; }
}
} // namespace jetpbrt

// ---- float image readers of FEnvironmentMap: files from outside, every offset checked against the bytes read ------------------------------
namespace jetpbrt
{
namespace
{
bool Refuse(std::string* error, const std::string& msg) { if (error) *error = msg; return false; }
bool ReadWhole(const char* filename, std::vector<uint8_t>& f)
{
	if (!filename) return false;
	std::ifstream in(filename, std::ios::binary);
	if (!in) return false;
	f.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	return true;
}
bool MapSizeOk(long w, long h) { return w >= 1 && w <= 4096 && h >= 1 && h <= 4096; }
bool TexelsOk(const std::vector<float>& rgb) { for (float v : rgb) if (!(v >= 0.f) || !std::isfinite(v)) return false; return true; }
}

bool ReadImagePFM(const char* filename, std::vector<float>& rgb, int& width, int& height, std::string* error)
{
	rgb.clear(); width = height = 0;
	std::vector<uint8_t> f;
	if (!ReadWhole(filename, f)) return Refuse(error, "cannot read the file");
	if (f.size() < 3 || f[0] != 'P' || (f[1] != 'F' && f[1] != 'f') || !std::isspace(f[2])) return Refuse(error, "not a PFM file");
	const int nch = f[1] == 'F' ? 3 : 1;
	size_t at = 2; long w = 0, h = 0;
	if (!PpmToken(f, at, w) || !PpmToken(f, at, h)) return Refuse(error, "PFM: bad size");
	if (!MapSizeOk(w, h)) return Refuse(error, "PFM: size out of range (1 .. 4096 per side)");
	// the scale line: a decimal number, negative for little-endian floats; one whitespace byte ends the header
	while (at < f.size() && (f[at] == ' ' || f[at] == '\t' || f[at] == '\r' || f[at] == '\n')) at++;
	const size_t s0 = at;
	while (at < f.size() && !std::isspace(f[at]) && at - s0 < 64) at++;
	if (at == s0 || at >= f.size() || !std::isspace(f[at])) return Refuse(error, "PFM: bad scale line");
	const std::string tok((const char*)&f[s0], at - s0);
	char* end = nullptr; const double scale = std::strtod(tok.c_str(), &end);
	if (end == tok.c_str() || *end != 0 || !(scale != 0.0) || !std::isfinite(scale)) return Refuse(error, "PFM: bad scale line");
	at++;
	const size_t n = (size_t)w * h, need = n * nch * 4;
	if (f.size() - at < need) return Refuse(error, "PFM: truncated");
	const bool little = scale < 0.0;
	rgb.resize(n * 3);
	for (long y = 0; y < h; y++)
		for (long x = 0; x < w; x++)
		{
			const uint8_t* p = &f[at + ((size_t)(h - 1 - y) * w + x) * nch * 4];          // the file's first row is the image's bottom row
			for (int k = 0; k < 3; k++)
			{
				const uint8_t* b = p + (nch == 3 ? 4 * k : 0);
				const uint32_t u = little ? ((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24))
				                          : ((uint32_t)b[3] | ((uint32_t)b[2] << 8) | ((uint32_t)b[1] << 16) | ((uint32_t)b[0] << 24));
				float v; std::memcpy(&v, &u, 4);
				rgb[3 * ((size_t)y * w + x) + k] = v;
			}
		}
	if (!TexelsOk(rgb)) { rgb.clear(); return Refuse(error, "PFM: a value is negative or not finite"); }
	width = (int)w; height = (int)h;
	return true;
}

bool ReadImageHDR(const char* filename, std::vector<float>& rgb, int& width, int& height, std::string* error)
{
	rgb.clear(); width = height = 0;
	std::vector<uint8_t> f;
	if (!ReadWhole(filename, f)) return Refuse(error, "cannot read the file");
	if (f.size() < 2 || f[0] != '#' || f[1] != '?') return Refuse(error, "not a Radiance HDR file");
	// header lines up to the empty one, then the resolution line
	size_t at = 0; bool blank = false, rgbe = false;
	while (at < f.size())
	{
		const size_t e = std::find(f.begin() + at, f.end(), (uint8_t)'\n') - f.begin();
		if (e >= f.size()) return Refuse(error, "HDR: truncated header");
		const std::string line((const char*)&f[at], e - at);
		at = e + 1;
		if (line.empty()) { blank = true; break; }
		if (line == "FORMAT=32-bit_rle_rgbe") rgbe = true;
	}
	if (!blank || !rgbe) return Refuse(error, "HDR: no FORMAT=32-bit_rle_rgbe header");
	const size_t e = std::find(f.begin() + std::min(at, f.size()), f.end(), (uint8_t)'\n') - f.begin();
	if (e >= f.size()) return Refuse(error, "HDR: truncated header");
	const std::string res((const char*)&f[at], e - at);
	at = e + 1;
	long h = 0, w = 0; char tail = 0;
	if (std::sscanf(res.c_str(), "-Y %ld +X %ld%c", &h, &w, &tail) != 2) return Refuse(error, "HDR: resolution line is not \"-Y h +X w\"");
	if (!MapSizeOk(w, h)) return Refuse(error, "HDR: size out of range (1 .. 4096 per side)");
	std::vector<uint8_t> px((size_t)w * h * 4);
	for (long y = 0; y < h; y++)
	{
		uint8_t* row = &px[(size_t)y * w * 4];
		if (w >= 8 && w < 32768 && f.size() - at >= 4 && f[at] == 2 && f[at + 1] == 2 && ((size_t)f[at + 2] << 8 | f[at + 3]) == (size_t)w)
		{   // a run-length encoded scanline: the four channels one after another, runs (count > 128: count - 128 copies) and literals
			at += 4;
			for (int k = 0; k < 4; k++)
				for (long x = 0; x < w;)
				{
					if (at >= f.size()) return Refuse(error, "HDR: truncated");
					int cnt = f[at++];
					if (cnt > 128)
					{
						cnt -= 128;
						if (cnt > w - x || at >= f.size()) return Refuse(error, "HDR: bad run");
						const uint8_t v = f[at++];
						for (int i = 0; i < cnt; i++) row[4 * (x++) + k] = v;
					}
					else
					{
						if (cnt == 0 || cnt > w - x || f.size() - at < (size_t)cnt) return Refuse(error, "HDR: bad run");
						for (int i = 0; i < cnt; i++) row[4 * (x++) + k] = f[at++];
					}
				}
		}
		else
		{
			if (f.size() - at < (size_t)w * 4) return Refuse(error, "HDR: truncated");
			std::memcpy(row, &f[at], (size_t)w * 4); at += (size_t)w * 4;
		}
	}
	rgb.resize((size_t)w * h * 3);
	for (size_t i = 0; i < (size_t)w * h; i++)
	{
		const uint8_t* p = &px[4 * i];
		const float s = p[3] ? std::ldexp(1.0f, (int)p[3] - (128 + 8)) : 0.f;              // byte * 2^(e - 128) / 256
		rgb[3 * i] = p[0] * s; rgb[3 * i + 1] = p[1] * s; rgb[3 * i + 2] = p[2] * s;
	}
	if (!TexelsOk(rgb)) { rgb.clear(); return Refuse(error, "HDR: a value is not finite"); }
	width = (int)w; height = (int)h;
	return true;
}

static unsigned long long NextMapId() { static std::atomic<unsigned long long> n{ 0 }; return ++n; }

FEnvironmentMap::FEnvironmentMap(const float* rgb, int w, int h) : id(NextMapId())
{
	if (rgb && MapSizeOk(w, h)) { data.assign(rgb, rgb + (size_t)w * h * 3); width = w; height = h; }
}

std::shared_ptr<FEnvironmentMap> FEnvironmentMap::FromFile(const char* filename, std::string* error)
{
	std::vector<uint8_t> head;
	{
		std::ifstream in(filename ? filename : "", std::ios::binary);
		if (!in) { Refuse(error, "cannot read the file"); return nullptr; }
		char b[2] = { 0, 0 }; in.read(b, 2); head.assign(b, b + in.gcount());
	}
	std::vector<float> rgb; int w = 0, h = 0;
	if (head.size() == 2 && head[0] == 'P' && (head[1] == 'F' || head[1] == 'f')) { if (!ReadImagePFM(filename, rgb, w, h, error)) return nullptr; }
	else if (head.size() == 2 && head[0] == '#' && head[1] == '?') { if (!ReadImageHDR(filename, rgb, w, h, error)) return nullptr; }
	else
	{
		std::vector<uint8_t> b8;
		if (!ReadImageRGB8(filename, b8, w, h)) { Refuse(error, "not a PFM, Radiance HDR, binary PPM or uncompressed BMP file (or truncated)"); return nullptr; }
		if (!MapSizeOk(w, h)) { Refuse(error, "size out of range (1 .. 4096 per side)"); return nullptr; }
		rgb.resize(b8.size());
		for (size_t i = 0; i < b8.size(); i++) rgb[i] = (float)b8[i] / 255.f;
	}
	return std::make_shared<FEnvironmentMap>(rgb.data(), w, h);
}
} // namespace jetpbrt
