// djb_kernels_model_set_proxy.hip -- SGD / ABC model sets: the two per-hit steps of the dj_sgd / dj_abc plugins beyond eval / evalp, against
// the fitted tabular proxy of the hit's material (mitsuba/djb_mitsuba_model.hpp: the plugins build tabular(model, 90) and take sample() and
// pdf() from it):
//   k_model_set_evalp_is_proxy<KIND, DENSE>   k_evalp_is_proxy<KIND_TABULAR, KIND, DENSE> (djb_kernels_proxy.hip) per hit: direction from
//                                             mf_sample<KIND_TABULAR>, pdf from the pdf arm of mf_eval_pdf<KIND_TABULAR, 4>, weight =
//                                             divs(eval_one<KIND, 2>, pdf); i stored, weight 0 and pdf 0 where i.z <= 0 (a NaN i.z is evaluated)
//   k_model_set_evalp_pdf<KIND, DENSE>        k_evalp_pdf_proxy<KIND_TABULAR, KIND, DENSE> (djb_kernels_proxy_light.hip) per hit, for a GIVEN
//                                             pair: fr = eval_one<KIND, 2>, pdf = the same pdf arm; both +0 where i.z <= 0 || o.z <= 0
// KIND sgd / abc: eight kernels, in a translation unit of their own so that no other kernel's code moves.  The loop is k_model_set's
// (djb_kernels_model_set.hip): one hit per lane, workgroups of 256, workgroup-uniform k0, the staged exp / pow tables, rows in dynamic LDS
// or in global memory behind a workgroup-uniform switch, non-temporal streams (the id stream included).  A tabular proxy's table
// coordinates go through the arctangent core, so its table is staged for abc as well (ATANT in djb_kernels_proxy.hip).  The model side is
// k_model_set's `unit` (djb_model_set_unit.inc); the proxy side is a lane-private Brdf whose p22 / sigma / qf / n_qf are the hit's
// material's.  Nothing is re-derived, so an active hit has the bits of the single-material call with both params NULL.
//
// The proxy block (djb_model_set.hip): float tab[M][3][res] -- p22, sigma, qf of material m one after the other -- then int n_qf[M].  It is
// read from global memory; the lane's table pointers are the block's base plus a 32-bit byte offset: material * 12 res (+ the table's 4 res
// or 8 res), below 2^31 because M * res <= DJB_MODEL_SET_PROXY_MAX_ENTRIES = 2^27 (static_assert below); n_qf[m] sits at 12 M res + 4 m.  100 materials
// at res 90 are 108 KB: L2 resident.  No copy of the tables in LDS (not measured to pay).  cdf and the Fresnel spline are
// not in the block: mf_sample<KIND_TABULAR> reads qf alone (mf_sample_vp22_std -> tab_qf_radial), the pdf arm reads sigma (mf_sigma ->
// sigma_std_radial, for o, and for i under shadowing) and p22 (mf_ndf -> mf_p22 -> p22_radial); WANT = 4 never evaluates the Fresnel term,
// and tab_cdf_radial is called by the cdf query alone.
//
// Read for launch-uniform assumptions before a wave was allowed to mix materials -- a wave now holds n_qf = 90 next to n_qf = 2, finite
// tables next to tables with NaN:
//   spline_locate / spline_f   `n` is an int operand of per-lane arithmetic (a conversion, two clamps); the two table reads index with the
//                              clamped i1, i2 in [0, n - 1] whatever u is (NaN and out-of-range u convert to a clamped index), so a lane
//                              with n_qf = 2 reads qf[0], qf[1] of ITS row and nothing past them.  No loop, no readfirstlane.
//   tab_qf_radial              spline_f(b.qf, b.n_qf, u), then tan_fast_f: per lane.  n_qf is a loop bound nowhere on these two paths (the
//                              loops over it are the fitter's).
//   sigma_std_radial / p22_radial<KIND_TABULAR>   spline_f on b.sigma / b.p22 with b.n_sigma / b.n_p22 = res: launch-uniform here, as there.
//   mf_eval_pdf<KIND_TABULAR, 4>   b.shadow is the one value it branches on: launch-uniform here too (one fit serves the whole set).
//   mf_sample<KIND_TABULAR>    reads pp (launch-uniform: params::standard()) and qf; its GlibcTabs argument is Beckmann's and unused.
//   stage_table                not used: it stages ONE table for the workgroup and redirects the pointer, which is what a set cannot do.
//   the pointers               formed per lane from the id; n_qf[m] is a vector load.  None of these functions contains a readfirstlane or a
//                              scalar load of a count: the compiler may only prove uniform what is a kernel argument (res, shadow, pp).
// Read once in the ISA of the eight kernels: there is no flat_load, no scratch access and no readfirstlane.  Rows are ds_read_b64 /
// global_load_dwordx2 and n_qf[m] is a global_load_dword, both with the base in SGPRs and a 32-bit VGPR offset.  The table entries are
// global_load_dword too, but with a 64-bit VGPR address: spline_f indexes pts[i1] with a sign-extended int, so the lane's 32-bit table offset
// is widened before the entry's index is added (74 such loads in the eight kernels).  Changing that means changing spline_f, which every
// tabular kernel shares (profiles/model_set_proxy/kernel_resources.txt).
//
// Inactive hits (id outside [0, M)) and lanes past the end of the batch form no address from the id and read nothing; an inactive hit stores
// +0 in every output, and so does a light-sample hit below the horizon, which reads neither row nor table.  A wave without an active lane
// skips the arithmetic.  Every lane reads its hit before it writes it.  Bytes per hit: sampling 4 + 4 + 4 + 12 read, 12 + 12 + 4 written
// (52); light sample 4 + 12 + 12 read, 12 + 4 written (44).
#include "djb_internal.hpp"
#include <string.h>

using namespace djbdev;

namespace {

constexpr int BLOCK = 256;
constexpr long long GRID_CAP = 256LL * 16;                 // as k_model_set: one trip of the grid is GRID_CAP * BLOCK = 1 048 576 hits
static_assert(GRID_CAP * BLOCK == djbk::MODEL_SET_PROXY_TRIP, "the trip size the tests restate");

#include "djb_hit_source.inc"                              // BatchHits
// min_waves(kind, true), registers (tools/kernel_resources.sh, profiles/model_set_proxy/kernel_resources.txt): the sampled direction, o and
// the pdf live across eval_one next to the per-lane row.  sgd: 141 (dense) / 143 (strided) VGPRs, 3 waves per SIMD (k_model_set<SGD>: 124 / 127
// at 4); at the hint 4 all four sgd kernels kept 48 / 64 bytes of scratch at 128 VGPRs.  abc: 77 (dense: 6 waves) / 83 (strided: 5 waves)
// against k_model_set<ABC>'s 64 / 70 at 8 / 7; at the hint 6 the strided forms kept 16 bytes of scratch, at 7 all four kept 32 / 48.  The hints
// are the largest without scratch; nothing was timed against them.
// rows_lds(kind, true), the LDS budget for rows next to 5248 B of staged tables (exp 2048, pow 3072, arctangent 128): sgd 101 rows at 3
// workgroups per CU, as k_model_set (the 100 published rows fit); abc 211 rows at 8 workgroups per CU (k_model_set: 213 -- the arctangent
// table is staged here)
#include "djb_model_hits.inc"                              // row_stride, unit, rows_lds, min_waves, ModelLaunch, stage, proxy_of, model_is_trip

template <int KIND, bool DENSE>
__global__ __launch_bounds__(BLOCK, min_waves(KIND, true)) void k_model_set_evalp_is_proxy(Brdf b, Params pp, ModelSetProxy px, const double *rows, int n_mat, int in_lds,
                                                                                           long long n, const int32_t *mat, const float *u1a, const float *u2a,
                                                                                           View vo, View vw_out, View vi_out, float *out_pdf)
{
	__shared__ unsigned long long s_exp[256];
	__shared__ double s_pow[384];
	__shared__ double s_atan[16];
	extern __shared__ double s_rows[];                                            // n_mat * STRIDE doubles when in_lds, else none
	const BatchHits<DENSE, true, true> src(n, mat, n_mat);
	b = stage<KIND, true>(b, s_exp, s_pow, s_atan, s_rows, rows, src.n_mat, in_lds);
	const long long stride = src.stride();
	for (long long j0 = src.start(); j0 < src.count(); j0 += stride)                      // j0: workgroup-uniform
		model_is_trip<KIND>(src, j0, s_rows, b, pp, px, rows, in_lds, u1a, u2a, vo, vw_out, vi_out, out_pdf);
}

// the light sample: written out, as k_scene_model_light is -- on one body the pair did not keep its instructions
template <int KIND, bool DENSE>
__global__ __launch_bounds__(BLOCK, min_waves(KIND, true)) void k_model_set_evalp_pdf(Brdf b, Params pp, ModelSetProxy px, const double *rows, int n_mat, int in_lds,
                                                                                long long n, const int32_t *mat, View vi, View vo, View vout, float *out_pdf)
{
	constexpr unsigned int STRIDE = (unsigned int)row_stride(KIND);
	__shared__ unsigned long long s_exp[256];
	__shared__ double s_pow[384];
	__shared__ double s_atan[16];
	extern __shared__ double s_rows[];
	b = stage<KIND, true>(b, s_exp, s_pow, s_atan, s_rows, rows, (unsigned int)n_mat, in_lds);
	const long long stride = (long long)gridDim.x * BLOCK;
	const unsigned int t = threadIdx.x;
	for (long long k0 = (long long)blockIdx.x * BLOCK; k0 < n; k0 += stride) {     // k0: workgroup-uniform
		const long long k = k0 + t;
		const bool live = k < n;
		bool act = false;
		unsigned int id = 0u;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		if (live) {                                                                // 44 B per hit, touched once: non-temporal
			const unsigned int raw = (unsigned int)__builtin_nontemporal_load(mat + k);
			const unsigned int toff = lane_byte_offset(t);
			i = DENSE ? load3_dense_off_nt(vi, k0, toff) : load3(vi, k); o = DENSE ? load3_dense_off_nt(vo, k0, toff) : load3(vo, k);
			// active and above the horizon (the plugins' guard; a NaN z is evaluated): anything else reads neither row nor table
			act = raw < (unsigned int)n_mat && !(i.z <= 0.0f || o.z <= 0.0f);
			id = act ? raw : 0u;
		}
		v3 fr = mk(0, 0, 0); float pdf = 0.0f;                                     // inactive, or below the horizon: +0
		if (__ballot(act) != 0ull) {                                               // wave-uniform
			if (act) {
				const Brdf pb = proxy_of(b, px, (unsigned int)n_mat, id);
				v3 unused;
				mf_eval_pdf<KIND_TABULAR, 4>(pb, pp, i, o, unused, pdf);
				if (in_lds) unit<KIND, 2>(b, s_rows + id * STRIDE, i, o, fr);
				else unit<KIND, 2>(b, (const double *)((const char *)rows + (size_t)(id * (STRIDE * 8u))), i, o, fr);
			}
		}
		if (live) {
			const unsigned int soff = lane_byte_offset(t);
			if (DENSE) { __builtin_nontemporal_store(pdf, dense_off(out_pdf + k0, soff)); store3_dense_off_nt(vout, k0, soff, fr); }
			else { __builtin_nontemporal_store(pdf, out_pdf + k); store3(vout, k, fr); }
		}
	}
}

template <int KIND>
hipError_t launch_is(hipStream_t s, const ModelSetProxy &p, const Params &pp, const double *rows, int n_mat, bool rows_global, long long n,
                     const int32_t *mat, const float *u1, const float *u2, const View &o, const View &out_w, const View &out_i, float *out_pdf)
{
	const ModelLaunch L(KIND, n_mat, rows_global, true);
	const dim3 g(djbk::grid_capped(n, BLOCK, GRID_CAP));
	if (djbk::dense_strict(o) && djbk::dense_strict(out_w) && djbk::dense_strict(out_i))
		hipLaunchKernelGGL((k_model_set_evalp_is_proxy<KIND, true>), g, dim3(BLOCK), L.lds, s, L.b, pp, p, rows, n_mat, L.in_lds, n, mat, u1, u2, o, out_w, out_i, out_pdf);
	else
		hipLaunchKernelGGL((k_model_set_evalp_is_proxy<KIND, false>), g, dim3(BLOCK), L.lds, s, L.b, pp, p, rows, n_mat, L.in_lds, n, mat, u1, u2, o, out_w, out_i, out_pdf);
	return hipGetLastError();
}

template <int KIND>
hipError_t launch_pdf(hipStream_t s, const ModelSetProxy &p, const Params &pp, const double *rows, int n_mat, bool rows_global, long long n,
                      const int32_t *mat, const View &i, const View &o, const View &out, float *out_pdf)
{
	const ModelLaunch L(KIND, n_mat, rows_global, true);
	const dim3 g(djbk::grid_capped(n, BLOCK, GRID_CAP));
	if (djbk::dense_strict(i) && djbk::dense_strict(o) && djbk::dense_strict(out))
		hipLaunchKernelGGL((k_model_set_evalp_pdf<KIND, true>), g, dim3(BLOCK), L.lds, s, L.b, pp, p, rows, n_mat, L.in_lds, n, mat, i, o, out, out_pdf);
	else
		hipLaunchKernelGGL((k_model_set_evalp_pdf<KIND, false>), g, dim3(BLOCK), L.lds, s, L.b, pp, p, rows, n_mat, L.in_lds, n, mat, i, o, out, out_pdf);
	return hipGetLastError();
}

} // namespace

namespace djbk {

hipError_t launch_model_set_evalp_is_proxy(hipStream_t s, int kind, const double *rows, int n_mat, bool rows_global, const ModelSetProxy &proxy,
                                           const Params &proxy_p, long long n, const int32_t *material, const float *u1, const float *u2,
                                           const View &o, const View &out_w, const View &out_i, float *out_pdf)
{
	if (n <= 0) return hipSuccess;
	if (kind == KIND_SGD) return launch_is<KIND_SGD>(s, proxy, proxy_p, rows, n_mat, rows_global, n, material, u1, u2, o, out_w, out_i, out_pdf);
	if (kind == KIND_ABC) return launch_is<KIND_ABC>(s, proxy, proxy_p, rows, n_mat, rows_global, n, material, u1, u2, o, out_w, out_i, out_pdf);
	return hipErrorInvalidValue;
}

hipError_t launch_model_set_evalp_pdf(hipStream_t s, int kind, const double *rows, int n_mat, bool rows_global, const ModelSetProxy &proxy,
                                      const Params &proxy_p, long long n, const int32_t *material, const View &i, const View &o,
                                      const View &out_fr, float *out_pdf)
{
	if (n <= 0) return hipSuccess;
	if (kind == KIND_SGD) return launch_pdf<KIND_SGD>(s, proxy, proxy_p, rows, n_mat, rows_global, n, material, i, o, out_fr, out_pdf);
	if (kind == KIND_ABC) return launch_pdf<KIND_ABC>(s, proxy, proxy_p, rows, n_mat, rows_global, n, material, i, o, out_fr, out_pdf);
	return hipErrorInvalidValue;
}

} // namespace djbk
