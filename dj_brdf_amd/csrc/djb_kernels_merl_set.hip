// djb_kernels_merl_set.hip -- MERL material sets: a batch of hits that lands on M resident MERL tables, one launch.
//
// The bin of a MERL look-up depends on (i, o) alone (merl_index_fast / merl_index), never on the material: a mixed batch computes
// the index once and gathers from table[material][index].  No kind dispatch, no divergence beyond the one the single-material kernels
// have.  Three kernels, all with the two-tier shape of k_merl_fast (djb_kernels_merl.hip) and k_evalp_is_proxy<.., KIND_MERL, ..>
// (djb_kernels_proxy.hip): tier 1 in place, the pairs it declines wait in a per-wave LDS queue -- the record carries the material id --
// and one drain site finishes them with the exact index as dense waves.
//   k_merl_set_fast<WANT>                      eval (WANT 1) / evalp (WANT 2) per hit
//   k_evalp_is_proxy_merl_set<PKIND, DENSE>    the per-bounce step of dj_merl per hit: direction and pdf from a GGX or Beckmann lobe
//                                              whose Params come per lane from the resident Params[M], f_r cos from table[material]
//   k_merl_set_evalp_pdf<PKIND, DENSE>         the light-sample step of dj_merl per hit, for a GIVEN pair: f_r cos from table[material] and
//                                              the proxy lobe's pdf with Params[material], both +0 where i or o is not above the horizon
// A hit whose id is outside [0, M) is inactive: every output is +0.0f, no table or parameter entry is read, nothing is queued.
// The per-unit functions are the ones the single-material kernels call (mf_sample, the pdf arm of mf_eval_pdf, merl_index_fast,
// merl_index, scale, divs), so an active hit has the bits of the single-material route.
// Addressing: material * 1458000 + index fits an int32 up to DJB_MERL_SET_MAX = 1024 tables, the BYTE offset (x 12) does not beyond
// table 245 -- merl_set_texel forms the element index in 64 bits.
#include "djb_internal.hpp"
#include "djb_worklist.hpp"

using namespace djbdev;

namespace {

constexpr int BLOCK = 256;
constexpr long long GRID_CAP = 256LL * 16;
constexpr long long MERL_TEXELS = 90LL * 90 * 180;

DJB_DEV v3 merl_set_texel(const MerlTexel *tex, unsigned int material, int idx)
{
	const MerlTexel t = tex[(unsigned long long)material * (unsigned long long)MERL_TEXELS + (unsigned long long)(unsigned int)idx];
	return mk(t.x, t.y, t.z);
}

// the queue of the pairs tier 1 declines (djb_worklist.hpp: recq_push / recq_drain).  The part of a record all three kernels share:
// {k lo, k hi, material, i.xyz, o.xyz}
DJB_DEV void rec_pack(unsigned int *rec, long long k, unsigned int material, v3 i, v3 o)
{
	rec_put_k(rec, k); rec[2] = material; rec_put_v3(rec, 3, i); rec_put_v3(rec, 6, o);
}

// ---- eval / evalp.  DENSE: every view has stride 1 -- the 40 B/hit streams (id, i, o, out) are touched once: non-temporal, so that
// they leave the L2 to the table gathers
template <int WANT, bool DENSE>
__global__ __launch_bounds__(BLOCK) void k_merl_set_fast(const MerlTexel *tex, int n_mat, long long n, const int32_t *mat, View vi, View vo, View vout,
                                                         MerlGuard g, int merl_exact)
{
	__shared__ unsigned int s_q[BLOCK / 64][9][RECQ_CAP];
	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	unsigned int (&q)[9][RECQ_CAP] = s_q[wave];
	unsigned int qn = 0;                                                           // wave-uniform
	const long long stride = (long long)gridDim.x * BLOCK;
	for (long long k0 = (long long)blockIdx.x * BLOCK; ; k0 += stride) {           // workgroup-uniform trip count; one extra trip flushes the queues
		const bool last = k0 >= n;
		bool amb = false;
		unsigned int id = 0u;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		const long long k = k0 + t;
		const unsigned int rem = last ? 0u : n - k0 >= (long long)BLOCK ? (unsigned int)BLOCK : (unsigned int)(n - k0);
		if (t < rem) {
			id = (unsigned int)__builtin_nontemporal_load(mat + k);
			i = DENSE ? load3_dense_nt(vi, k0, t) : load3(vi, k); o = DENSE ? load3_dense_nt(vo, k0, t) : load3(vo, k);
			v3 fr = mk(0, 0, 0);                                                       // an inactive hit: +0, nothing read
			if (id < (unsigned int)n_mat) {                                            // negative ids are >= 2^31 as unsigned
				int idx = 0;
				if (!merl_exact && merl_index_fast(i, o, g, idx)) {
					const v3 e = merl_set_texel(tex, id, idx);
					fr = (WANT & 2) ? scale(i.z, e) : e;                                   // brdf::evalp, dj_brdf.h:803-806
				} else amb = true;                                                      // the exact index finishes this pair
			}
			if (!amb) { if (DENSE) store3_dense_nt(vout, k0, t, fr); else store3(vout, k, fr); }
		}
		unsigned int rec[9];                                                       // built here, outside the branches above (djb_worklist.hpp)
		rec_pack(rec, k, id, i, o);
		recq_push(q, qn, lane, amb, rec);
		recq_drain(q, qn, lane, last, [&](const unsigned int *r) {
			const v3 i = rec_v3(r, 3);
			const v3 e = merl_set_texel(tex, r[2], merl_index(i, rec_v3(r, 6)));
			store3(vout, rec_k(r), (WANT & 2) ? scale(i.z, e) : e);
		});
		if (last) break;
	}
}

// ---- proxy importance sampling per hit: k_evalp_is_proxy<PKIND, KIND_MERL, DENSE> with Params and the table base per lane
template <int PKIND, bool DENSE>
__global__ __launch_bounds__(BLOCK) void k_evalp_is_proxy_merl_set(Brdf pb, const Params *params, const MerlTexel *tex, int n_mat, long long n,
                                                                   const int32_t *mat, const float *u1a, const float *u2a, View vo, View vw_out,
                                                                   View vi_out, float *out_pdf, MerlGuard g, int merl_exact)
{
	static_assert(PKIND == KIND_GGX || PKIND == KIND_BECKMANN, "the proxy of a MERL set is an analytic lobe");
	constexpr bool GLIBCT = PKIND == KIND_BECKMANN;                                // logf / expf / powf of Beckmann's quantile functions
	__shared__ double s_glibc[GLIBCT ? GLIBC_LDS_WORDS : 1];
	__shared__ unsigned long long s_exp[GLIBCT ? 256 : 1];
	__shared__ unsigned int s_q[BLOCK / 64][10][RECQ_CAP];
	GlibcTabs gt = glibc_tabs_global();
	if (GLIBCT) {
		gt = glibc_tabs_to_lds(s_glibc, threadIdx.x, BLOCK);
		const LdsTab e = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
		pb.exp_lds = e; gt.exp64 = e;
		__syncthreads();
	}
	pb.atan_lds = 0u;

	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	unsigned int (&q)[10][RECQ_CAP] = s_q[wave];
	unsigned int qn = 0;                                                           // wave-uniform
	const long long stride = (long long)gridDim.x * BLOCK;
	for (long long k0 = (long long)blockIdx.x * BLOCK; ; k0 += stride) {           // one extra trip flushes the queues
		const bool last = k0 >= n;
		bool amb = false;
		unsigned int id = 0u;
		v3 i_ = mk(0, 0, 0), o = mk(0, 0, 1); float pdf = 0.0f;                        // an inactive hit: +0 everywhere, nothing read
		const long long k = k0 + t;
		const unsigned int rem = last ? 0u : n - k0 >= (long long)BLOCK ? (unsigned int)BLOCK : (unsigned int)(n - k0);
		if (t < rem) {
			id = (unsigned int)__builtin_nontemporal_load(mat + k);
			v3 w = mk(0, 0, 0);
			if (id < (unsigned int)n_mat) {
				const unsigned int toff = lane_byte_offset(t);
				const float u1 = DENSE ? (*dense_off(u1a + k0, toff)) : u1a[k];
				const float u2 = DENSE ? (*dense_off(u2a + k0, toff)) : u2a[k];
				o = DENSE ? load3_dense_off(vo, k0, toff) : load3(vo, k);
				const Params pp = params[id];
				// ---- proxy: direction, then the pdf-only arm of mf_eval_pdf on (i, o)
				i_ = mf_sample<PKIND>(pb, pp, u1, u2, o, gt);
				if (!(i_.z <= 0.0f)) {                                                  // the side check; a NaN i.z is evaluated
					v3 unused;
					mf_eval_pdf<PKIND, 4>(pb, pp, i_, o, unused, pdf);
					int idx = 0;
					if (!merl_exact && merl_index_fast(i_, o, g, idx))
						w = divs(scale(i_.z, merl_set_texel(tex, id, idx)), pdf);           // brdf::evalp = eval * i.z, dj_brdf.h:803-806
					else amb = true;                                                    // the exact index finishes this pair (below)
				}
			}
			const unsigned int soff = lane_byte_offset(t);                             // again: the stores sit in another block than the loads
			if (DENSE) { store3_dense_off(vi_out, k0, soff, i_); (*dense_off(out_pdf + k0, soff)) = pdf; }
			else { store3(vi_out, k, i_); out_pdf[k] = pdf; }
			if (!amb) { if (DENSE) store3_dense_off(vw_out, k0, soff, w); else store3(vw_out, k, w); }
		}
		unsigned int rec[10];
		rec_pack(rec, k, id, i_, o); rec[9] = __float_as_uint(pdf);
		recq_push(q, qn, lane, amb, rec);
		recq_drain(q, qn, lane, last, [&](const unsigned int *r) {
			const v3 iq = rec_v3(r, 3);
			const v3 e = merl_set_texel(tex, r[2], merl_index(iq, rec_v3(r, 6)));
			store3(vw_out, rec_k(r), divs(scale(iq.z, e), __uint_as_float(r[9])));
		});
		if (last) break;
	}
}

// ---- the light sample (next-event estimation / MIS) per hit: for a given pair, evalp from table[material] and the proxy's pdf with
// params[material]; dj_merl::eval / ::pdf return 0 where cosTheta(wi) <= 0 || cosTheta(wo) <= 0 (a NaN z is evaluated).  The pdf needs
// no table: it is stored at once and the queue's record is the 9 words of k_merl_set_fast.  The texel of a pair tier 1 decides is asked
// for BEFORE the pdf arithmetic and consumed after it.  Beckmann: the pdf arm calls exp alone -- its table is staged, the log / pow
// tables of mf_sample are not.
template <int PKIND, bool DENSE>
__global__ __launch_bounds__(BLOCK) void k_merl_set_evalp_pdf(Brdf pb, const Params *params, const MerlTexel *tex, int n_mat, long long n,
                                                              const int32_t *mat, View vi, View vo, View vout, float *out_pdf, MerlGuard g,
                                                              int merl_exact)
{
	static_assert(PKIND == KIND_GGX || PKIND == KIND_BECKMANN, "the proxy of a MERL set is an analytic lobe");
	constexpr bool EXPT = PKIND == KIND_BECKMANN;
	__shared__ unsigned long long s_exp[EXPT ? 256 : 1];
	__shared__ unsigned int s_q[BLOCK / 64][9][RECQ_CAP];
	if (EXPT) {
		pb.exp_lds = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
		__syncthreads();
	}
	pb.atan_lds = 0u;

	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	unsigned int (&q)[9][RECQ_CAP] = s_q[wave];
	unsigned int qn = 0;                                                           // wave-uniform
	const long long stride = (long long)gridDim.x * BLOCK;
	for (long long k0 = (long long)blockIdx.x * BLOCK; ; k0 += stride) {           // workgroup-uniform trip count; one extra trip flushes the queues
		const bool last = k0 >= n;
		bool amb = false;
		unsigned int id = 0u;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		const long long k = k0 + t;
		const unsigned int rem = last ? 0u : n - k0 >= (long long)BLOCK ? (unsigned int)BLOCK : (unsigned int)(n - k0);
		if (t < rem) {
			id = (unsigned int)__builtin_nontemporal_load(mat + k);
			i = DENSE ? load3_dense_nt(vi, k0, t) : load3(vi, k); o = DENSE ? load3_dense_nt(vo, k0, t) : load3(vo, k);
			v3 fr = mk(0, 0, 0); float pdf = 0.0f;                                     // inactive, or below the horizon: +0, nothing read
			if (id < (unsigned int)n_mat && !(i.z <= 0.0f || o.z <= 0.0f)) {           // dj_merl.cpp:57-60, 69-72; a NaN z is evaluated
				const Params pp = params[id];                                           // asked for first: loads return in order, and the
				int idx = 0;                                                            // pdf must not wait for the texel behind them
				const bool decided = !merl_exact && merl_index_fast(i, o, g, idx);
				v3 e = mk(0, 0, 0);
				if (decided) e = merl_set_texel(tex, id, idx);                          // in flight across the pdf
				v3 unused;
				mf_eval_pdf<PKIND, 4>(pb, pp, i, o, unused, pdf);                       // microfacet::pdf, dj_brdf.h:1713-1730
				if (decided) fr = scale(i.z, e);                                        // brdf::evalp, dj_brdf.h:803-806
				else amb = true;                                                        // the exact index finishes this pair
			}
			if (DENSE) __builtin_nontemporal_store(pdf, dense_at(out_pdf + k0, t)); else __builtin_nontemporal_store(pdf, out_pdf + k);
			if (!amb) { if (DENSE) store3_dense_nt(vout, k0, t, fr); else store3(vout, k, fr); }
		}
		unsigned int rec[9];                                                       // built here, outside the branches above (djb_worklist.hpp)
		rec_pack(rec, k, id, i, o);
		recq_push(q, qn, lane, amb, rec);
		recq_drain(q, qn, lane, last, [&](const unsigned int *r) {
			const v3 iq = rec_v3(r, 3);
			const v3 e = merl_set_texel(tex, r[2], merl_index(iq, rec_v3(r, 6)));
			store3(vout, rec_k(r), scale(iq.z, e));
		});
		if (last) break;
	}
}

template <int WANT>
hipError_t launch_set_eval(hipStream_t s, const MerlTexel *tex, int n_mat, long long n, const int32_t *mat, const View &i, const View &o,
                           const View &out, bool merl_exact)
{
	const MerlGuard g = MERL_GUARD_DEFAULT;
	dim3 grid(djbk::grid_capped(n, BLOCK, GRID_CAP)), block(BLOCK);
	if (djbk::dense_strict(i) && djbk::dense_strict(o) && djbk::dense_strict(out))
		hipLaunchKernelGGL((k_merl_set_fast<WANT, true>), grid, block, 0, s, tex, n_mat, n, mat, i, o, out, g, merl_exact ? 1 : 0);
	else
		hipLaunchKernelGGL((k_merl_set_fast<WANT, false>), grid, block, 0, s, tex, n_mat, n, mat, i, o, out, g, merl_exact ? 1 : 0);
	return hipGetLastError();
}

template <int PKIND>
hipError_t launch_set_proxy(hipStream_t s, const Brdf &pb, const Params *params, const MerlTexel *tex, int n_mat, long long n, const int32_t *mat,
                            const float *u1, const float *u2, const View &o, const View &out_w, const View &out_i, float *out_pdf, bool merl_exact)
{
	const MerlGuard g = MERL_GUARD_DEFAULT;
	dim3 grid(djbk::grid_capped(n, BLOCK, GRID_CAP)), block(BLOCK);
	if (djbk::dense_strict(o) && djbk::dense_strict(out_w) && djbk::dense_strict(out_i))
		hipLaunchKernelGGL((k_evalp_is_proxy_merl_set<PKIND, true>), grid, block, 0, s, pb, params, tex, n_mat, n, mat, u1, u2, o, out_w, out_i, out_pdf, g, merl_exact ? 1 : 0);
	else
		hipLaunchKernelGGL((k_evalp_is_proxy_merl_set<PKIND, false>), grid, block, 0, s, pb, params, tex, n_mat, n, mat, u1, u2, o, out_w, out_i, out_pdf, g, merl_exact ? 1 : 0);
	return hipGetLastError();
}

template <int PKIND>
hipError_t launch_set_evalp_pdf(hipStream_t s, const Brdf &pb, const Params *params, const MerlTexel *tex, int n_mat, long long n, const int32_t *mat,
                                const View &i, const View &o, const View &out, float *out_pdf, bool merl_exact)
{
	const MerlGuard g = MERL_GUARD_DEFAULT;
	dim3 grid(djbk::grid_capped(n, BLOCK, GRID_CAP)), block(BLOCK);
	if (djbk::dense_strict(i) && djbk::dense_strict(o) && djbk::dense_strict(out))
		hipLaunchKernelGGL((k_merl_set_evalp_pdf<PKIND, true>), grid, block, 0, s, pb, params, tex, n_mat, n, mat, i, o, out, out_pdf, g, merl_exact ? 1 : 0);
	else
		hipLaunchKernelGGL((k_merl_set_evalp_pdf<PKIND, false>), grid, block, 0, s, pb, params, tex, n_mat, n, mat, i, o, out, out_pdf, g, merl_exact ? 1 : 0);
	return hipGetLastError();
}

} // namespace

namespace djbk {

hipError_t launch_merl_set_eval(hipStream_t s, const djbdev::MerlTexel *tex, int n_mat, long long n, const int32_t *material, const View &i,
                                const View &o, const View &out, bool want_cos, bool merl_exact)
{
	if (n <= 0) return hipSuccess;
	return want_cos ? launch_set_eval<2>(s, tex, n_mat, n, material, i, o, out, merl_exact)
	                : launch_set_eval<1>(s, tex, n_mat, n, material, i, o, out, merl_exact);
}

hipError_t launch_merl_set_evalp_is_proxy(hipStream_t s, const Brdf &proxy, const Params *params, const djbdev::MerlTexel *tex, int n_mat, long long n,
                                          const int32_t *material, const float *u1, const float *u2, const View &o, const View &out_w,
                                          const View &out_i, float *out_pdf, bool merl_exact)
{
	if (n <= 0) return hipSuccess;
	switch (proxy.kind) {
	case KIND_GGX: return launch_set_proxy<KIND_GGX>(s, proxy, params, tex, n_mat, n, material, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	case KIND_BECKMANN: return launch_set_proxy<KIND_BECKMANN>(s, proxy, params, tex, n_mat, n, material, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	}
	return hipErrorInvalidValue;
}

hipError_t launch_merl_set_evalp_pdf(hipStream_t s, const Brdf &proxy, const Params *params, const djbdev::MerlTexel *tex, int n_mat, long long n,
                                     const int32_t *material, const View &i, const View &o, const View &out_fr, float *out_pdf, bool merl_exact)
{
	if (n <= 0) return hipSuccess;
	switch (proxy.kind) {
	case KIND_GGX: return launch_set_evalp_pdf<KIND_GGX>(s, proxy, params, tex, n_mat, n, material, i, o, out_fr, out_pdf, merl_exact);
	case KIND_BECKMANN: return launch_set_evalp_pdf<KIND_BECKMANN>(s, proxy, params, tex, n_mat, n, material, i, o, out_fr, out_pdf, merl_exact);
	}
	return hipErrorInvalidValue;
}

} // namespace djbk
