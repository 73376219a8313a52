// djb_device_units.inc -- part of djb_device.hpp (included inside namespace djbdev): array access, the counter-based RNG of the
// synthetic workloads, one unit of each batch operator (eval_one, sample_one, pp_one, query_one ...), the MERL / UTIA table converters.
// ------------------------------------------------------------------ array access
DJB_DEV v3 load3(const View &v, long long k)
{
	long long off = k * v.stride;
	return mk(v.x[off], v.y[off], v.z[off]);
}
DJB_DEV void store3(const View &v, long long k, v3 a)
{
	long long off = k * v.stride;
	v.x[off] = a.x; v.y[off] = a.y; v.z[off] = a.z;
}

// Dense batches (every view SoA with stride 1: what device-resident callers and bench.py pass) address their arrays
// as  uniform base pointer (SGPRs: array + first unit of the workgroup) + 32-bit lane offset,  which costs one
// VALU shift for all ten arrays of a kernel; the generic strided form spends ~35 VALU instructions per pair on 64-bit
// index arithmetic (k * stride per component), 10 % of the GGX eval+pdf kernel.  k0 is workgroup-uniform.
// (the lane offset is formed in 32 bits -- t is a thread index, 4 t cannot wrap -- and only then widened: `base[t]` would shift the widened index,
// a 64-bit value the instruction selector no longer recognises as SGPR base + 32-bit VGPR offset: one v_lshl_add_u64 per access)
DJB_DEV const float *dense_at(const float *base, unsigned int t) { return (const float *)((const char *)base + (t << 2)); }
DJB_DEV float *dense_at(float *base, unsigned int t) { return (float *)((char *)base + (t << 2)); }
// ... and the widening must happen in the basic block of the access (instruction selection is per block): a kernel's batch loop takes
// its lane's byte offset through lane_byte_offset() once per iteration -- opaque, so that it is not hoisted out as a 64-bit value -- and
// addresses with dense_off()
#if defined(DJB_HOST_MATH)
DJB_DEV unsigned int lane_byte_offset(unsigned int t) { return t << 2; }
#else
DJB_DEV unsigned int lane_byte_offset(unsigned int t) { unsigned int o = t << 2; asm volatile("" : "+v"(o)); return o; }
#endif
DJB_DEV const float *dense_off(const float *base, unsigned int off) { return (const float *)((const char *)base + off); }
DJB_DEV float *dense_off(float *base, unsigned int off) { return (float *)((char *)base + off); }
DJB_DEV v3 load3_dense_off(const View &v, long long k0, unsigned int off) { return mk(*dense_off(v.x + k0, off), *dense_off(v.y + k0, off), *dense_off(v.z + k0, off)); }
DJB_DEV void store3_dense_off(const View &v, long long k0, unsigned int off, v3 a) { *dense_off(v.x + k0, off) = a.x; *dense_off(v.y + k0, off) = a.y; *dense_off(v.z + k0, off) = a.z; }
DJB_DEV v3 load3_dense(const View &v, long long k0, unsigned int t)
{
	const float *x = v.x + k0, *y = v.y + k0, *z = v.z + k0;
	return mk(*dense_at(x, t), *dense_at(y, t), *dense_at(z, t));
}
DJB_DEV void store3_dense(const View &v, long long k0, unsigned int t, v3 a)
{
	float *x = v.x + k0, *y = v.y + k0, *z = v.z + k0;
	*dense_at(x, t) = a.x; *dense_at(y, t) = a.y; *dense_at(z, t) = a.z;
}

// the same with the non-temporal hint (device): streams that are touched once, in a kernel whose table gathers want the XCD's L2 for themselves
#if !defined(DJB_HOST_MATH)
DJB_DEV v3 load3_dense_nt(const View &v, long long k0, unsigned int t)
{
	const float *x = v.x + k0, *y = v.y + k0, *z = v.z + k0;
	return mk(__builtin_nontemporal_load(dense_at(x, t)), __builtin_nontemporal_load(dense_at(y, t)), __builtin_nontemporal_load(dense_at(z, t)));
}
DJB_DEV void store3_dense_nt(const View &v, long long k0, unsigned int t, v3 a)
{
	float *x = v.x + k0, *y = v.y + k0, *z = v.z + k0;
	__builtin_nontemporal_store(a.x, dense_at(x, t)); __builtin_nontemporal_store(a.y, dense_at(y, t)); __builtin_nontemporal_store(a.z, dense_at(z, t));
}
// ... and addressed as SGPR base + the lane's 32-bit byte offset taken through lane_byte_offset() once per block of accesses.
// k_evalp_pdf_proxy uses them with a merl or utia target: there load3_dense_nt's addresses were kept as 64-bit values across the body
// (80 / 103 VGPRs against 63 / 85).  With an sgd or abc target it is the other way round -- the opaque offset costs 121 / 73 VGPRs
// against 92 / 59 -- so those keep load3_dense_nt / store3_dense_nt.  Register counts from the compiler's resource remarks; the two
// forms were not timed against each other.
DJB_DEV v3 load3_dense_off_nt(const View &v, long long k0, unsigned int off)
{
	return mk(__builtin_nontemporal_load(dense_off(v.x + k0, off)), __builtin_nontemporal_load(dense_off(v.y + k0, off)),
	          __builtin_nontemporal_load(dense_off(v.z + k0, off)));
}
DJB_DEV void store3_dense_off_nt(const View &v, long long k0, unsigned int off, v3 a)
{
	__builtin_nontemporal_store(a.x, dense_off(v.x + k0, off)); __builtin_nontemporal_store(a.y, dense_off(v.y + k0, off));
	__builtin_nontemporal_store(a.z, dense_off(v.z + k0, off));
}
#endif

// ------------------------------------------------------------------ counter-based RNG (synth.py)
DJB_DEV uint32_t pcg(uint32_t x)
{
	uint32_t state = x * 747796405u + 2891336453u;
	uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
	return (word >> 22u) ^ word;
}
DJB_DEV uint32_t hash_u32(uint32_t seed, uint64_t k, uint32_t c)
{
	uint32_t h = pcg(seed + c * 0x9E3779B9u);
	h = pcg(h ^ (uint32_t)(k & 0xFFFFFFFFull));
	h = pcg(h + (uint32_t)(k >> 32));
	return h;
}
// The on-chip uniforms of sample_rng / evalp_is_rng / djb_gen_uniforms (round 6; synth.rng_uniforms restates it in numpy).  One
// multiply-xorshift finaliser (the `lowbias32` constants: two odd multipliers, shifts 16 / 15 / 16; avalanche bias 0.17 %) over the
// Weyl-stepped counter keyed by a per-launch scalar: key = pcg(seed) is wave-uniform (scalar ALU), the counter's two words enter
// through multiplies shared by every stream of the sample.  12 VALU instructions per uniform + 3 shared where the three chained PCG
// rounds of hash_u32 took 35 -- the generator was ~70 of the 677 instructions of a Beckmann sample (profiles/archive/r05_NOTES.md section 2).  SURVEY 8(d) asks
// for a counter hash reproducible on CPU and GPU, nothing more; test inputs and golden vectors keep hash_u32 (synth.uniforms).
DJB_DEV uint32_t mix32(uint32_t x)
{
	x ^= x >> 16; x *= 0x7feb352du;
	x ^= x >> 15; x *= 0x846ca68bu;
	x ^= x >> 16;
	return x;
}
DJB_DEV float gen_uniform(uint32_t seed, uint64_t k)
{
	// Weyl step first: consecutive counters (lanes) must differ in more than their low bits when they reach the finaliser -- without the
	// multiply the pairs (u_k, u_k+1) and (u_k, u_k+64) fail a 64 x 64 chi-square by 18 and 30 sigma (tests/test_cpu_path.py holds the
	// restatement to that test).  The term is the same for every stream of a sample: one multiply-add shared by u1 and u2.
	const uint32_t w = (uint32_t)k * 0x9E3779B9u + (uint32_t)(k >> 32) * 0x85EBCA6Bu;
	return (float)(mix32(w + pcg(seed)) >> 8) * 5.9604644775390625e-08f;   // 2^-24
}
DJB_DEV v3 gen_direction(uint32_t seed, uint64_t k)
{
	float x = (float)(hash_u32(seed, k, 0) >> 8) * 1.1920928955078125e-07f - 1.0f;   // 2^-23
	float y = (float)(hash_u32(seed, k, 1) >> 8) * 1.1920928955078125e-07f - 1.0f;
	float r2 = x * x + y * y;
	if (r2 >= 0.998f) { x *= 0.5f; y *= 0.5f; }
	float z = sqrtf((1.0f - x * x) - y * y);
	return mk(x, y, z);
}

// ================================================================== one unit of each batch operator
// The bodies the kernels (djb_kernels_eval.hip) and the host loops (djb_cpu.cpp) both run, one (i, o) pair /
// sample / query per call.
template <int KIND, int WANT, int FRK = -1, bool STD = false>
DJB_DEV void eval_one(const Brdf &b, const Params &p, v3 i, v3 o, v3 &fr, float &pdf)
{
	if (DJB_IS_MICROFACET(KIND)) {
		mf_eval_pdf<KIND, WANT, FRK, STD>(b, p, i, o, fr, pdf);
	} else {
		if (WANT & 3) {
			v3 e;
			if (KIND == KIND_MERL) e = merl_eval(b, i, o);
			else if (KIND == KIND_UTIA) e = utia_eval(b, i, o);
			else if (KIND == KIND_SGD) e = sgd_eval(b, i, o);
			else if (KIND == KIND_ABC) e = abc_eval(b, i, o);
			else e = divs(mk(p.nx, p.ny, p.nz), F(DJB_PI));        // lambert: reflectance / M_PI, dj_brdf.h:861-868
			fr = (WANT & 2) ? scale(i.z, e) : e;                   // brdf::evalp, dj_brdf.h:803-806
		}
		if (WANT & 4) pdf = div_pi_to_f32(D(i.z));                 // brdf::pdf = float(double(i.z) / pi), dj_brdf.h:842-845
	}
}


// sample (IS == false) / evalp_is (IS == true) of one unit; FRK as in mf_eval_pdf
template <int KIND, bool IS, int FRK = -1>
DJB_DEV void sample_one(const Brdf &b, const Params &p, float u1, float u2, v3 o, const GlibcTabs &gt,
                        v3 &i_out, v3 &w_out, float &pdf_out)
{
	w_out = mk(0, 0, 0); pdf_out = 0.0f;
	if (DJB_IS_MICROFACET(KIND)) {
		if (!IS) i_out = mf_sample<KIND>(b, p, u1, u2, o, gt);
		else {
			i_out = mk(0, 0, 0);
			w_out = mf_evalp_is<KIND, FRK>(b, p, u1, u2, o, i_out, pdf_out, gt);
		}
	} else {
		// brdf::sample / brdf::evalp_is defaults (cosine hemisphere), dj_brdf.h:816-845
		float x, y;
		uniform_to_concentric(u1, u2, x, y);
		i_out = mk(x, y, F(sqrt(1.0 - D(x * x) - D(y * y))));
		if (IS) {
			v3 fr; float pdf;
			eval_one<KIND, 6>(b, p, i_out, o, fr, pdf);
			w_out = divs(fr, pdf);
			pdf_out = pdf;
		}
	}
}

// per-pair microfacet::params.  MODE 0: pdfparams record (ax, ay, rho, tx, ty); MODE 1: LEAN texel moments (E1..E5)
// composed with the surface's base lobe as the plugin does per hit: params = lrep_to_params(lrep(lean) * dmapscale +
// params_to_lrep(base))  (mitsuba/dj_beckmannconductor.cpp:296-314), optionally written back to out_pp5
DJB_DEV void pp_resolve(int mode, const float *r, const LeanCfg &lc, float *out_pp5,
                        float &ax, float &ay, float &rho, float &tx, float &ty)
{
	if (mode == 0) { ax = r[0]; ay = r[1]; rho = r[2]; tx = r[3]; ty = r[4]; }
	else {
		lrep_to_pdfparams(lean_compose(r, lc), ax, ay, rho, tx, ty);
		if (out_pp5) { out_pp5[0] = ax; out_pp5[1] = ay; out_pp5[2] = rho; out_pp5[3] = tx; out_pp5[4] = ty; }
	}
}
template <int KIND, int WANT, int MODE, int FRK = -1>
DJB_DEV void pp_one(const Brdf &b, v3 i, v3 o, const float *r, const LeanCfg &lc, float *out_pp5, v3 &fr, float &pdf)
{
	float ax, ay, rho, tx, ty;
	pp_resolve(MODE, r, lc, out_pp5, ax, ay, rho, tx, ty);
	Params p = params_from_pdfparams(ax, ay, rho, tx, ty);
	mf_eval_pdf<KIND, WANT, FRK>(b, p, i, o, fr, pdf);
}

// sample / evalp_is with per-pair params: what dj_beckmann_conductor::sample does per hit (mitsuba/dj_beckmannconductor.cpp:373-413)
template <int KIND, bool IS, int MODE, int FRK = -1>
DJB_DEV void pp_sample_one(const Brdf &b, float u1, float u2, v3 o, const float *r, const LeanCfg &lc, float *out_pp5,
                           const GlibcTabs &gt, v3 &i_out, v3 &w_out, float &pdf_out)
{
	float ax, ay, rho, tx, ty;
	pp_resolve(MODE, r, lc, out_pp5, ax, ay, rho, tx, ty);
	Params p = params_from_pdfparams(ax, ay, rho, tx, ty);
	sample_one<KIND, IS, FRK>(b, p, u1, u2, o, gt, i_out, w_out, pdf_out);
}

// ------------------------------------------------------------------ microfacet / radial queries
// (dj_brdf.h:258-276, 307-314).  `which` is wave-uniform.
enum { Q_NDF = 0, Q_GAF, Q_G1, Q_SIGMA, Q_P22, Q_VP22, Q_VNDF, Q_FRESNEL,
       Q_P22_RADIAL = 16, Q_SIGMA_STD_RADIAL, Q_CDF_RADIAL, Q_QF_RADIAL, Q_QF2_RADIAL, Q_QF3_RADIAL, Q_QF1,
       Q_A_PDF1 = 32, Q_A_CDF1, Q_A_QF1, Q_A_PDF2, Q_A_CDF2, Q_A_QF2,
       Q_MODEL_NDF = 48, Q_MODEL_GAF, Q_MODEL_G1 };


template <int KIND>
DJB_DEV v3 query_one(const Brdf &b, const Params &p, int which, long long k, const View &va, const View &vb, const View &vc)
{
	v3 a = load3(va, k);
	v3 r = mk(0, 0, 0);
	switch (which) {
	case Q_NDF: r.x = mf_ndf<KIND>(b, a, p); break;
	case Q_GAF: {   // gaf(h, i, o): a = h (unused by Smith), vb = i, vc = o
		v3 i = load3(vb, k), o = load3(vc, k);
		float g1o = mf_g1_from_sigma(o, mf_sigma<KIND>(b, o, p), p);
		float g1i = b.shadow ? mf_g1_from_sigma(i, mf_sigma<KIND>(b, i, p), p) : 0.0f;
		r.x = mf_gaf_from_g1(b.shadow, g1i, g1o); break;
	}
	case Q_G1: { v3 kk = load3(vb, k); r.x = mf_g1_from_sigma(kk, mf_sigma<KIND>(b, kk, p), p); break; }
	case Q_SIGMA: r.x = mf_sigma<KIND>(b, a, p); break;
	case Q_P22: r.x = mf_p22<KIND>(b, a.x, a.y, p); break;
	case Q_VP22: case Q_VNDF: {
		v3 kk = load3(vb, k);
		v3 h = which == Q_VNDF ? a : normalize(mk(-a.x, -a.y, 1));
		float kh = dot(kk, h);
		float vn = D(kh) > 0.0 ? kh * mf_ndf<KIND>(b, h, p) / mf_sigma<KIND>(b, kk, p) : 0.0f;
		r.x = which == Q_VNDF ? vn : (h.z * h.z * h.z) * vn; break;
	}
	case Q_FRESNEL: r = fresnel_eval(b.fr, a.x); break;
	case Q_P22_RADIAL: r.x = p22_radial<KIND>(b, a.x); break;
	case Q_SIGMA_STD_RADIAL: r.x = sigma_std_radial<KIND>(b, a.x); break;
	case Q_CDF_RADIAL: r.x = cdf_radial<KIND>(b, a.x); break;
	case Q_QF_RADIAL: r.x = qf_radial<KIND>(b, a.x); break;
#if defined(DJB_HOST_MATH)
	case Q_QF2_RADIAL: if (KIND == KIND_USER) { r.x = user_ndf(b).qf2_radial(user_ndf(b).user, a.x, a.y, a.z); break; }
	                   r.x = KIND == KIND_BECKMANN ? beckmann_qf2_radial(a.x, a.y, a.z, glibc_tabs_global())
	                       : KIND == KIND_GGX ? ggx_qf2_radial(a.x, a.y, a.z) : 0.0f; break;
	case Q_QF3_RADIAL: if (KIND == KIND_USER) { r.x = user_ndf(b).qf3_radial(user_ndf(b).user, a.x, a.y); break; }
	                   r.x = KIND == KIND_BECKMANN ? beckmann_qf1(a.x, glibc_tabs_global())
	                       : KIND == KIND_GGX ? ggx_qf3_radial(a.x, a.y) : 0.0f; break;
#else
	case Q_QF2_RADIAL: r.x = KIND == KIND_BECKMANN ? beckmann_qf2_radial(a.x, a.y, a.z, glibc_tabs_global())
	                       : KIND == KIND_GGX ? ggx_qf2_radial(a.x, a.y, a.z) : 0.0f; break;
	case Q_QF3_RADIAL: r.x = KIND == KIND_BECKMANN ? beckmann_qf1(a.x, glibc_tabs_global())
	                       : KIND == KIND_GGX ? ggx_qf3_radial(a.x, a.y) : 0.0f; break;
#endif
	case Q_QF1: r.x = KIND == KIND_BECKMANN ? beckmann_qf1(a.x, glibc_tabs_global()) : KIND == KIND_GGX ? ggx_qf1(a.x) : 0.0f; break;
	// tabular_anisotropic::{pdf1, cdf1, qf1, pdf2, cdf2, qf2} (dj_brdf.h:450-455)
	case Q_A_PDF1: r.x = KIND == KIND_TABULAR_ANISO ? aniso_pdf1(b, a.x) : 0.0f; break;
	case Q_A_CDF1: r.x = KIND == KIND_TABULAR_ANISO ? aniso_cdf1(b, a.x) : 0.0f; break;
	case Q_A_QF1:  r.x = KIND == KIND_TABULAR_ANISO ? aniso_qf1(b, a.x) : 0.0f; break;
	case Q_A_PDF2: r.x = KIND == KIND_TABULAR_ANISO ? aniso_pdf2(b, a.x, a.y) : 0.0f; break;
	case Q_A_CDF2: r.x = KIND == KIND_TABULAR_ANISO ? aniso_cdf2(b, a.x, a.y) : 0.0f; break;
	case Q_A_QF2:  r.x = KIND == KIND_TABULAR_ANISO ? aniso_qf2(b, a.x, a.y) : 0.0f; break;
	}
	return r;
}

// sgd::{ndf, gaf, g1, fresnel} and abc::{ndf, gaf, fresnel} (dj_brdf.h:505-509, 530-533)
template <int KIND>
DJB_DEV v3 model_query_one(const Brdf &b, int which, long long k, const View &va, const View &vb, const View &vc)
{
	v3 a = load3(va, k), r = mk(0, 0, 0);
	switch (which) {
	case Q_FRESNEL: r = fresnel_eval(b.fr, a.x); break;
	case Q_MODEL_NDF: r = KIND == KIND_SGD ? sgd_ndf_rgb(b, a) : abc_ndf_rgb(b, a); break;
	case Q_MODEL_GAF: {
		v3 i = load3(vb, k), o = load3(vc, k);
		if (KIND == KIND_SGD) r = sgd_gaf_rgb(b, i, o);
		else r.x = abc_gaf(a, i, o);
		break;
	}
	case Q_MODEL_G1: if (KIND == KIND_SGD) r = sgd_g1_rgb(b, a); break;
	}
	return r;
}

// dj_brdf.h:1010-1023 applied once per table entry instead of once per lookup: n = 1458000 texels from 3*n doubles
DJB_DEV MerlTexel merl_convert_one(const double *s, long long n, long long k)
{
	float r = F(s[k] * (1.00 / 1500.0));
	float g = F(s[k + n] * (1.15 / 1500.0));
	float b = F(s[k + 2 * n] * (1.66 / 1500.0));
	if (D(r) < 0.0 || D(g) < 0.0 || D(b) < 0.0) r = g = b = 0.0f;
	MerlTexel t; t.x = r; t.y = g; t.z = b;
	return t;
}

// utia::normalize (dj_brdf.h:1162-1177) then the (float_t) cast of dj_brdf.h:1144: record e of the 288*288
// records of eight float4 (see utia_eval); n = 3*288*288 samples (three planes)
DJB_DEV void utia_convert_one(const double *s, long long n, long long e, float4 *table)
{
	const float kf = 1.f / 140.f;
	const long long plane = n / 3;
	// e = 288 * (48 * iti + ipi) + 48 * itv + ipv
	long long ipv = e % 48, itv = (e / 48) % 6, row = e / 288, ipi = row % 48;
	float t[32];
	for (int c = 0; c < 2; ++c)
		for (int k = 0; k < 2; ++k)
			for (int l = 0; l < 2; ++l) {
				long long tv = itv + c > 5 ? 5 : itv + c;
				long long src = 288 * (row - ipi + (ipi + k) % 48) + 48 * tv + (ipv + l) % 48;
				for (int ch = 0; ch < 3; ++ch) {
					double v = s[ch * plane + src] > 0.0 ? s[ch * plane + src] : 0.0;
					t[3 * (4 * c + 2 * k + l) + ch] = F(v * D(kf));
				}
			}
	for (int j = 24; j < 32; ++j) t[j] = 0.0f;
	for (int j = 0; j < 8; ++j) { float4 q; q.x = t[4 * j]; q.y = t[4 * j + 1]; q.z = t[4 * j + 2]; q.w = t[4 * j + 3]; table[8 * e + j] = q; }
}

