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
// The three bodies live in djb_merl_hits.inc, written once over a hit source (djb_hit_source.inc): here the batch, in the scene kernels the
// list of the scene's MERL hits.
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

#include "djb_hit_source.inc"                              // BatchHits
#include "djb_merl_hits.inc"                               // merl_set_texel, the queue record, merl_eval_hits / merl_is_hits / merl_light_hits

// ---- eval / evalp.  DENSE: every view has stride 1 -- the 40 B/hit streams (id, i, o, out) are touched once: non-temporal, so that
// they leave the L2 to the table gathers
template <int WANT, bool DENSE>
__global__ __launch_bounds__(BLOCK) void k_merl_set_fast(const MerlTexel *tex, int n_mat, long long n, const int32_t *mat, View vi, View vo, View vout,
                                                         MerlGuard g, int merl_exact)
{
	__shared__ unsigned int s_q[BLOCK / 64][9][RECQ_CAP];
	merl_eval_hits<WANT>(BatchHits<DENSE, false, true>(n, mat, n_mat), s_q, tex, vi, vo, vout, g, merl_exact);
}

// ---- proxy importance sampling per hit.  The streams are read inside the active branch, the lane's offset through lane_byte_offset()
template <int PKIND, bool DENSE>
__global__ __launch_bounds__(BLOCK) void k_evalp_is_proxy_merl_set(Brdf pb, const Params *params, const MerlTexel *tex, int n_mat, long long n,
                                                                   const int32_t *mat, const float *u1a, const float *u2a, View vo, View vw_out,
                                                                   View vi_out, float *out_pdf, MerlGuard g, int merl_exact)
{
	constexpr bool GLIBCT = PKIND == KIND_BECKMANN;
	__shared__ double s_glibc[GLIBCT ? GLIBC_LDS_WORDS : 1];
	__shared__ unsigned long long s_exp[GLIBCT ? 256 : 1];
	__shared__ unsigned int s_q[BLOCK / 64][10][RECQ_CAP];
	merl_is_hits<PKIND>(BatchHits<DENSE, true, false>(n, mat, n_mat), s_glibc, s_exp, s_q, pb, params, tex, u1a, u2a, vo, vw_out, vi_out, out_pdf, g,
	                    merl_exact);
}

// ---- the light sample (next-event estimation / MIS) per hit
template <int PKIND, bool DENSE>
__global__ __launch_bounds__(BLOCK) void k_merl_set_evalp_pdf(Brdf pb, const Params *params, const MerlTexel *tex, int n_mat, long long n,
                                                              const int32_t *mat, View vi, View vo, View vout, float *out_pdf, MerlGuard g,
                                                              int merl_exact)
{
	__shared__ unsigned long long s_exp[PKIND == KIND_BECKMANN ? 256 : 1];
	__shared__ unsigned int s_q[BLOCK / 64][9][RECQ_CAP];
	merl_light_hits<PKIND>(BatchHits<DENSE, false, true>(n, mat, n_mat), s_exp, s_q, pb, params, tex, vi, vo, vout, out_pdf, g, merl_exact);
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
