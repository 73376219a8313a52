// djb_leanmap.inc -- LEAN maps (Olano & Baker 2010; the textures dj_beckmannconductor reads per hit): the per-texel code of the
// builders, the mip pyramid and the filtered lookup.  One source for the gfx950 kernels (djb_leanmap.hip, the MODE 2 per-pair
// kernels of djb_kernels_eval.hip) and for the host path (djb_cpu.cpp), as everything else in djb_device.hpp.
//
// Level 0 is the arithmetic of the reference's tools, operation for operation (utils/dmap2nmap.cpp:13-44, utils/nmap2leanmap.cpp:18-56).
// The pyramid and the filter have no reference (the reference leaves them to Mitsuba): include/djb_hip.h defines them as float
// operations in a fixed order, and this is that definition.
//
// Storage: one texel = 8 floats = 32 bytes, 32-byte aligned: E1 E2 E3 E4 | E5 0 0 0.  A tap of the filter is one dwordx4 and one
// dword from the same 32-byte sector (random gathers on this chip are bound by the number of requests, DESIGN.md 4.1).  Levels are
// stored one after the other, level 0 first; the map holds the UNBIASED moments.

struct LeanMap {
	const float4 *texels;     // 2 float4 per texel
	int lw, lh;               // log2 of the width / height of level 0
};
enum { LEANMAP_MAX_LOG2 = 13 };
// the layout of the pyramid is host code too (allocation, the per-level launches)
#if defined(DJB_HOST_MATH)
#define DJB_LAYOUT static inline
#else
#define DJB_LAYOUT __host__ __device__ __forceinline__
#endif                                            // 8192

DJB_LAYOUT int leanmap_levels(int lw, int lh) { return 1 + (lw > lh ? lw : lh); }
// texels before level l, l in [0, levels - 1]: levels 0 .. min(lw, lh) shrink by 4, the rest (one side is 1 texel) by 2
DJB_LAYOUT unsigned int leanmap_level_offset(int lw, int lh, int l)
{
	const int m = lw < lh ? lw : lh, M = lw < lh ? lh : lw;
	const int a = l < m ? l : m;
	const unsigned int wh4 = 4u << (lw + lh);                              // <= 2^28
	unsigned int off = (wh4 - (wh4 >> (2 * a))) / 3u;
	if (l > m) off += (2u << (M - m)) - (2u << (M - l));
	return off;
}
DJB_LAYOUT unsigned int leanmap_total_texels(int lw, int lh) { return leanmap_level_offset(lw, lh, leanmap_levels(lw, lh) - 1) + 1u; }

// ------------------------------------------------------------------ level 0
// dmap2nmap(), utils/dmap2nmap.cpp:20-43: CImg's atXY clamps at the border (Neumann); the conversions to uint8_t truncate
DJB_DEV unsigned char leanmap_to_u8(float t) { return t >= 0.0f && t < 256.0f ? (unsigned char)(int)t : (unsigned char)0; }
DJB_DEV void dmap_to_nmap_texel(const unsigned char *dmap, int w, int h, int i, int j, float scale, unsigned char *rgb)
{
	const int il = i > 0 ? i - 1 : 0, ir = i < w - 1 ? i + 1 : w - 1, jt = j > 0 ? j - 1 : 0, jb = j < h - 1 ? j + 1 : h - 1;
	const float z_l = (float)dmap[il + (long long)w * j] / 255.f, z_r = (float)dmap[ir + (long long)w * j] / 255.f;
	const float z_b = (float)dmap[i + (long long)w * jb] / 255.f, z_t = (float)dmap[i + (long long)w * jt] / 255.f;
	const float slope_x = (float)w * 0.5f * scale * (z_r - z_l);
	const float slope_y = (float)h * 0.5f * scale * (z_t - z_b);
	const float nrm_sqr = 1.f + slope_x * slope_x + slope_y * slope_y;
	const float nrm_inv = F(1.0 / sqrt(D(nrm_sqr)));
	const float nx = -slope_x * nrm_inv, ny = -slope_y * nrm_inv, nz = nrm_inv;
	const float tmp1 = F(0.5 * D(nx) + 0.5), tmp2 = F(0.5 * D(ny) + 0.5);
	rgb[0] = leanmap_to_u8(tmp1 * 255.0f);
	rgb[1] = leanmap_to_u8(tmp2 * 255.0f);
	rgb[2] = leanmap_to_u8(nz * 255.0f);
}
// nmap2leanmap(), utils/nmap2leanmap.cpp:33-54: a blue byte of 0 gives infinite (or NaN) moments, as there
DJB_DEV void nmap_to_lean_texel(unsigned char px_r, unsigned char px_g, unsigned char px_b, float base_roughness, float *e)
{
	const float tmp1 = ((float)px_r / 255.f) * 2.0f - 1.0f;
	const float tmp2 = ((float)px_g / 255.f) * 2.0f - 1.0f;
	const float tmp3 = ((float)px_b / 255.f);
	const float slope_x = -tmp1 / tmp3, slope_y = -tmp2 / tmp3;
	const float base_roughness_sqr = 0.5f * base_roughness * base_roughness;
	e[0] = slope_x; e[1] = slope_y;
	e[2] = slope_x * slope_x + base_roughness_sqr;
	e[3] = slope_y * slope_y + base_roughness_sqr;
	e[4] = slope_x * slope_y;
}
DJB_DEV void leanmap_store(float4 *t, const float *e)
{
	float4 a, b;
	a.x = e[0]; a.y = e[1]; a.z = e[2]; a.w = e[3];
	b.x = e[4]; b.y = 0.0f; b.z = 0.0f; b.w = 0.0f;
	t[0] = a; t[1] = b;
}
DJB_DEV void leanmap_fetch(const float4 *t, float *e)
{
	const float4 a = t[0];
	const float e5 = t[1].x;
	e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = e5;
}

// ------------------------------------------------------------------ pyramid
// texel (x, y) of a level of wd x hd texels from the level below it (ws x hs): the mean of the 2x2 block, the block clamped where
// the source is one texel wide or high; ((T00 + T10) + (T01 + T11)) * 0.25f per moment
DJB_DEV void leanmap_downsample_texel(const float4 *src, int ws, int hs, int x, int y, float *e)
{
	const int x0 = 2 * x < ws - 1 ? 2 * x : ws - 1, x1 = 2 * x + 1 < ws - 1 ? 2 * x + 1 : ws - 1;
	const int y0 = 2 * y < hs - 1 ? 2 * y : hs - 1, y1 = 2 * y + 1 < hs - 1 ? 2 * y + 1 : hs - 1;
	float t00[5], t10[5], t01[5], t11[5];
	leanmap_fetch(src + 2 * (x0 + (long long)ws * y0), t00);
	leanmap_fetch(src + 2 * (x1 + (long long)ws * y0), t10);
	leanmap_fetch(src + 2 * (x0 + (long long)ws * y1), t01);
	leanmap_fetch(src + 2 * (x1 + (long long)ws * y1), t11);
	for (int c = 0; c < 5; ++c) e[c] = ((t00[c] + t10[c]) + (t01[c] + t11[c])) * 0.25f;
}

// ------------------------------------------------------------------ filtered lookup
// the fraction of a texture coordinate: u - floorf(u); 0 where that is not in [0, 1) (NaN, inf, and a tiny negative u, whose
// fraction rounds up to 1)
DJB_DEV float leanmap_frac(float u)
{
	const float f = u - floorf(u);
	return f >= 0.0f && f < 1.0f ? f : 0.0f;
}
// the four taps of one level and their weights
struct LeanTaps { const float4 *t00, *t10, *t01, *t11; float fx, fy; };
DJB_DEV LeanTaps leanmap_taps(const LeanMap &m, int l, float uf, float vf)
{
	const int lwl = m.lw > l ? m.lw - l : 0, lhl = m.lh > l ? m.lh - l : 0;
	const int wl = 1 << lwl, hl = 1 << lhl;
	const float x = uf * (float)wl - 0.5f, y = vf * (float)hl - 0.5f;
	const float x0 = floorf(x), y0 = floorf(y);
	const int ix = (int)x0, iy = (int)y0;                                  // -1 .. wl - 1
	const unsigned int c0 = (unsigned int)ix & (unsigned int)(wl - 1), c1 = (unsigned int)(ix + 1) & (unsigned int)(wl - 1);   // repeat
	const unsigned int r0 = (unsigned int)iy & (unsigned int)(hl - 1), r1 = (unsigned int)(iy + 1) & (unsigned int)(hl - 1);
	const float4 *lev = m.texels + 2ull * leanmap_level_offset(m.lw, m.lh, l);
	LeanTaps t;
	t.t00 = lev + 2u * (c0 + (r0 << lwl)); t.t10 = lev + 2u * (c1 + (r0 << lwl));
	t.t01 = lev + 2u * (c0 + (r1 << lwl)); t.t11 = lev + 2u * (c1 + (r1 << lwl));
	t.fx = x - x0; t.fy = y - y0;
	return t;
}
// A = lerp(lerp(T00, T10, fx), lerp(T01, T11, fx), fy) per moment, lerp(a, b, s) = a + (b - a) * s: this form returns a where
// b == a and where s == 0 (finite taps), so a constant map filters to its constant and a texel centre to its texel, exactly --
// a (1 - s) + b s does neither
DJB_DEV float leanmap_lerp(float a, float b, float s) { return a + (b - a) * s; }
DJB_DEV void leanmap_bilinear(const LeanTaps &t, float *a)
{
	float t00[5], t10[5], t01[5], t11[5];
	leanmap_fetch(t.t00, t00); leanmap_fetch(t.t10, t10); leanmap_fetch(t.t01, t01); leanmap_fetch(t.t11, t11);
	for (int c = 0; c < 5; ++c) a[c] = leanmap_lerp(leanmap_lerp(t00[c], t10[c], t.fx), leanmap_lerp(t01[c], t11[c], t.fx), t.fy);
}
// the record (E1..E5) at (u, v, lod): bilinear in the two levels around lod, wrapped by repeat, then linear between them.
// lod: NaN -> 0, clamped to [0, levels - 1].  With an integral lod the upper level is not read.
DJB_DEV void leanmap_lookup(const LeanMap &m, float u, float v, float lod, float *r)
{
	const int top = leanmap_levels(m.lw, m.lh) - 1;
	if (!(lod == lod)) lod = 0.0f;
	lod = lod < 0.0f ? 0.0f : lod > (float)top ? (float)top : lod;
	const float lf = floorf(lod);
	const int l0 = (int)lf;
	const float t = lod - lf;
	const float uf = leanmap_frac(u), vf = leanmap_frac(v);
	leanmap_bilinear(leanmap_taps(m, l0, uf, vf), r);
	if (t != 0.0f) {
		float b[5];
		leanmap_bilinear(leanmap_taps(m, l0 + 1 < top ? l0 + 1 : top, uf, vf), b);
		for (int c = 0; c < 5; ++c) r[c] = leanmap_lerp(r[c], b[c], t);
	}
}
// where the per-hit callers take their records from: n (u, v) pairs and n lods (NULL: level 0)
struct LeanSrc { LeanMap map; const float *uv, *lod; };
DJB_DEV void leanmap_lookup_hit(const LeanSrc &s, long long k, float *r) { leanmap_lookup(s.map, s.uv[2 * k], s.uv[2 * k + 1], s.lod ? s.lod[k] : 0.0f, r); }
