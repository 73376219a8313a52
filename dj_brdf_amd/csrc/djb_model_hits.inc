// djb_model_hits.inc -- the per-hit SGD / ABC eval and sampling bodies, each written once over a hit source (djb_hit_source.inc): the set kernels of
// djb_kernels_model_set.hip / djb_kernels_model_set_proxy.hip run them on a batch, the scene kernels of djb_kernels_scene.hip /
// djb_kernels_scene_proxy.hip on the list of the scene's sgd or abc hits; and what those kernels' launchers share.  Included inside each
// file's anonymous namespace, after BLOCK and the source.  The kernels keep their __shared__ arrays and pass them in.
// A body is one TRIP of the grid-stride loop; the kernel holds the loop, the early exit and the call of stage() (djb_hit_source.inc says
// why).  The loop is k_eval's: one hit per lane, a workgroup-uniform j0, the staged exp / pow tables, rows in dynamic LDS or in global
// memory behind a workgroup-uniform switch.  An inactive hit and a lane past the end form no address from the id and read nothing; a wave without an active
// lane skips the arithmetic; every lane reads its hit before it writes it.
#include "djb_model_set_unit.inc"                          // row_stride, unit

// Two sets of budgets.  PROXY false, the eval / evalp kernels (the reasoning: djb_kernels_model_set.hip): 5248 B (sgd) / 5128 B (abc) of
// staged tables; PROXY true, the sampling and light-sample kernels (djb_kernels_model_set_proxy.hip): the arctangent table is staged for
// abc as well, and the proxy's registers lower the occupancy hints -- the largest without scratch.
constexpr int rows_lds(int kind, bool proxy) { return kind == KIND_SGD ? 101 : proxy ? 211 : 213; }      // the LDS budget, in rows
constexpr int min_waves(int kind, bool proxy) { return proxy ? (kind == KIND_SGD ? 3 : 5) : (kind == KIND_SGD ? 4 : 7); }
static_assert(2048 + 3072 + 128 + 8 * rows_lds(KIND_SGD, false) * row_stride(KIND_SGD) <= 163840 / 3, "sgd: three workgroups per CU");
static_assert(2048 + 3072 + 8 + 8 * rows_lds(KIND_ABC, false) * row_stride(KIND_ABC) <= 163840 / 8, "abc: eight workgroups per CU");
static_assert(2048 + 3072 + 128 + 8 * rows_lds(KIND_SGD, true) * row_stride(KIND_SGD) <= 163840 / 3, "sgd, proxy: three workgroups per CU");
static_assert(2048 + 3072 + 128 + 8 * rows_lds(KIND_ABC, true) * row_stride(KIND_ABC) <= 163840 / 8, "abc, proxy: eight workgroups per CU");
static_assert(65536ull * 8ull * (unsigned long long)row_stride(KIND_SGD) < (1ull << 31), "the byte offset of the last row fits 32 bits");
static_assert(12ull * (unsigned long long)djbk::MODEL_SET_PROXY_MAX_ENTRIES + 4ull * 65536ull < (1ull << 31), "the byte offset of the last table entry and of n_qf[M - 1] fits 31 bits");

using djbk::ModelSetProxy;                                 // the launch-uniform part of a set's proxy block: base, res, shadow

// the host side of a launch: the kind's Brdf, and whether the rows go to (dynamic) LDS -- a small set costs no occupancy
struct ModelLaunch {
	Brdf b; int in_lds; size_t lds;
	ModelLaunch(int kind, int n_mat, bool rows_global, bool proxy)
	{
		memset(&b, 0, sizeof b);
		b.kind = kind;
		b.fr.kind = kind == KIND_SGD ? FR_SGD : FR_UNPOLARIZED;
		in_lds = !rows_global && n_mat <= rows_lds(kind, proxy);
		lds = in_lds ? sizeof(double) * (size_t)n_mat * (size_t)row_stride(kind) : 0;
	}
};

// the staging prologue: exp and pow for the model, the arctangent core's for sgd and -- ATAN -- for a tabular proxy's table coordinates; the
// rows when in_lds (n_mat <= rows_lds: the launcher's test); the barrier
template <int KIND, bool ATAN>
DJB_DEV Brdf stage(Brdf b, unsigned long long *s_exp, double *s_pow, double *s_atan, double *s_rows, const double *rows, unsigned int n_mat, int in_lds)
{
	b.exp_lds = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
	b.pow_lds = glibc_pow_tab_to_lds(s_pow, threadIdx.x, BLOCK);
	b.atan_lds = ATAN ? atan_tab_to_lds(s_atan, threadIdx.x) : 0u;
	if (in_lds) {
		const unsigned int count = n_mat * (unsigned int)row_stride(KIND);
		for (unsigned int j = threadIdx.x; j < count; j += BLOCK) s_rows[j] = rows[j];
	}
	__syncthreads();
	return b;
}

// the lane's proxy: b's staged tables, the tables and the count of material `id`.  The block is float tab[M][3][res], then int n_qf[M]
DJB_DEV Brdf proxy_of(Brdf b, const ModelSetProxy &px, unsigned int n_mat, unsigned int id)
{
	const unsigned int res4 = (unsigned int)px.res * 4u;
	const char *base = (const char *)px.tab;
	const unsigned int off = id * (3u * res4);                                     // < 2^31 (above)
	b.shadow = px.shadow;
	b.p22 = (const float *)(base + off);
	b.sigma = (const float *)(base + (off + res4));
	b.qf = (const float *)(base + (off + 2u * res4));
	b.n_p22 = b.n_sigma = px.res;
	b.n_qf = *(const int *)(base + (n_mat * (3u * res4) + (id << 2)));
	return b;
}

// ---- eval (WANT 1) / evalp (WANT 2) per hit
template <int KIND, int WANT, class S>
DJB_DEV void model_eval_trip(const S &src, typename S::index j0, const double *s_rows, const Brdf &b, const double *rows, int in_lds, const View &vi,
                             const View &vo, const View &vout)
{
	typedef typename S::index index;
	constexpr unsigned int STRIDE = (unsigned int)row_stride(KIND);
	const unsigned int t = threadIdx.x;
	const bool live = (index)(j0 + t) < src.count();
	bool act = false;
	unsigned int id = 0u;
	index k = src.idle(j0, t);
	v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
	if (live) {
		k = src.at(j0, t);
		act = src.id(k, id);
		const typename S::lane_t l = src.lane(j0, t, k);
		i = src.in3(vi, l); o = src.in3(vo, l);
		if (!act) id = 0u;
	}
	v3 fr = mk(0, 0, 0);                                                           // an inactive hit: +0
	if (__ballot(act) != 0ull) {                                                   // wave-uniform: a wave of dead hits computes nothing
		if (act) {
			if (in_lds) unit<KIND, WANT>(b, s_rows + id * STRIDE, i, o, fr);                            // workgroup-uniform: ds_read_b64 ...
			else unit<KIND, WANT>(b, (const double *)((const char *)rows + (size_t)(id * (STRIDE * 8u))), i, o, fr);   // ... or uniform base + 32-bit byte offset
		}
	}
	if (live) src.out3(vout, src.lane(j0, t, k, true), fr);
}

// ---- sampling per hit: direction from mf_sample<KIND_TABULAR> on the hit's fitted proxy, pdf from the pdf arm of mf_eval_pdf, weight =
// divs(unit<KIND, 2>, pdf); i stored, weight 0 and pdf 0 where i.z <= 0 (a NaN i.z is evaluated)
template <int KIND, class S>
DJB_DEV void model_is_trip(const S &src, typename S::index j0, const double *s_rows, const Brdf &b, const Params &pp, const ModelSetProxy &px,
                           const double *rows, int in_lds, const float *u1a, const float *u2a, const View &vo, const View &vw_out, const View &vi_out,
                           float *out_pdf)
{
	typedef typename S::index index;
	constexpr unsigned int STRIDE = (unsigned int)row_stride(KIND);
	const GlibcTabs gt = glibc_tabs_global();                                     // Beckmann's: mf_sample<KIND_TABULAR> does not read it
	const unsigned int t = threadIdx.x;
	const bool live = (index)(j0 + t) < src.count();
	bool act = false;
	unsigned int id = 0u;
	index k = src.idle(j0, t);
	float u1 = 0.0f, u2 = 0.0f;
	v3 o = mk(0, 0, 1);
	if (live) {
		k = src.at(j0, t);
		act = src.id(k, id);
		const typename S::lane_t l = src.lane(j0, t, k);
		u1 = src.in1(u1a, l); u2 = src.in1(u2a, l);
		o = src.in3(vo, l);
		if (!act) id = 0u;
	}
	v3 w = mk(0, 0, 0), i_ = mk(0, 0, 0); float pdf = 0.0f;                        // an inactive hit: +0 everywhere
	if (__ballot(act) != 0ull) {                                                   // wave-uniform
		if (act) {
			const Brdf pb = proxy_of(b, px, src.n_mat, id);
			i_ = mf_sample<KIND_TABULAR>(pb, pp, u1, u2, o, gt);
			if (!(i_.z <= 0.0f)) {                                                  // the plugins' side check; a NaN i.z is evaluated
				v3 unused, fr = mk(0, 0, 0);
				mf_eval_pdf<KIND_TABULAR, 4>(pb, pp, i_, o, unused, pdf);
				if (in_lds) unit<KIND, 2>(b, s_rows + id * STRIDE, i_, o, fr);
				else unit<KIND, 2>(b, (const double *)((const char *)rows + (size_t)(id * (STRIDE * 8u))), i_, o, fr);
				w = divs(fr, pdf);                                                  // (1.0f / pdf) * fr: the IEEE result for a zero pdf
			}
		}
	}
	if (live) {
		const typename S::lane_t l = src.lane(j0, t, k);                            // again: the stores sit in another block than the loads
		src.out3(vi_out, l, i_); src.out1(out_pdf, l, pdf); src.out3(vw_out, l, w);
	}
}
