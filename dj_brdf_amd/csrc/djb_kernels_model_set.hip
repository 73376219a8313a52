// djb_kernels_model_set.hip -- SGD / ABC model sets: a batch of hits that lands on M resident parameter rows of ONE kind, eval / evalp per hit.
//
// For the single-material kernels (k_eval<KIND_SGD / KIND_ABC>, djb_kernels_eval.hip) the row is launch-uniform: b.model is one pointer,
// its doubles are scalar loads and SGPR operands.  Here the row moves with the hit's id, so every coefficient is per-lane data: a load
// per use (ds_read_b64 from the copy in LDS, global_load_dwordx2 otherwise) into a VGPR pair.  Nothing else changes:
//   k_model_set<KIND, WANT, DENSE>   KIND sgd / abc, WANT 1 eval / 2 evalp: one hit per lane, k_eval's loop shape, k_eval's staged tables
//                                    (exp and pow, the arctangent core's for sgd), eval_one<KIND, WANT> -- the function k_eval calls -- on a
//                                    lane-private Brdf whose `model` is the hit's row and whose Fresnel operands are that row's
// so an active hit has the bits of the single-material call.  The path was read for launch-uniform assumptions: sgd_g1_rgb / sgd_ndf_rgb
// branch on m[SGD_FAST_FLAG] (now a divergent branch: a wave that mixes rows runs both sides, each lane its own), fresnel_eval tests
// a[0] == a[1] == a[2] per lane, the fma_sk addends are literals, fdiv_r is not on this path, and nothing reads a row value from one lane.
// A translation unit of its own: the code of k_eval does not move with this one.
//
// rows = double[M][STRIDE], built on the host exactly as create_model builds the single row (djb_model_set.hip): STRIDE = SGD_FAST_ROW
// = 61 for sgd (the 33 doubles, then the constants of the decided fast tier; [33] = 0 for a row outside that tier's domain), 9 for abc.
// Both strides are odd: rows start 2 (mod 4) banks apart for the 64-bank ds_read_b64, so lanes that read one coefficient of different
// rows spread over 32 bank pairs.  The byte offset material * STRIDE * 8 is below 2^25 at DJB_MODEL_SET_MAX = 65536: 32-bit offsets.
// The Fresnel operands are converted per lane, (float)row[12 + c] / (float)row[15 + c] (sgd) and (float)row[8] (abc): create_model's conversions.
//
// Rows in LDS.  When M <= rows_lds(KIND, false) the workgroup copies the block into (dynamic) LDS once and the lanes read their coefficients from
// there; the launch asks for M * STRIDE * 8 bytes, so a small set costs no occupancy.  The budget is what the kind's occupancy leaves of
// the CU's 160 KiB next to the staged tables (5248 B sgd, 5128 B abc):
//   sgd  its 124 / 127 VGPRs allow 4 waves per SIMD (k_eval<SGD> runs 5 at 87) = 4 workgroups per CU up to 73 rows of 488 B; the budget
//        is 101 rows = 3 workgroups per CU (54613 B each, 49365 B for rows), so that the 100 published rows fit: measured at M = 100,
//        random ids, 4.42 ms per 1e8 hits from LDS at 3 workgroups against 7.49 ms from global memory at 4
//   abc  8 waves per SIMD (as k_eval<ABC>) = 8 workgroups per CU: 20480 B each, 15352 B for rows = 213 rows of 72 B
// Larger sets, and every set under DJB_OPT_MODEL_SET_ROWS_GLOBAL, read their rows from global memory (L2 / Infinity-Cache resident): 15-50 %
// slower where both were measured.  The branch is workgroup-uniform (a kernel argument); each side is eval_one inlined with pointers of
// one address space (ds_read_b64 / global_load_dwordx2 with the set's base in SGPRs; no flat loads).
//
// A hit whose id is outside [0, M) is inactive, as is a lane past the end of the batch: +0.0f in the three outputs (nothing, past the
// end), no address formed from its id, no row read; a wave without an active lane skips the arithmetic.  Every lane reads its hit before
// it writes it: index-aligned in-place calls are supported.  Streams are non-temporal: 4 (id) + 24 + 12 = 40 B per hit.
#include "djb_internal.hpp"
#include <string.h>

using namespace djbdev;

namespace {

constexpr int BLOCK = 256;
constexpr long long GRID_CAP = 256LL * 16;                 // as k_eval for these kinds (djb_kernels_eval.hip)

#include "djb_hit_source.inc"                              // BatchHits
// rows_lds(kind, false): the LDS budget, in rows (above).  min_waves(kind, false), registers (tools/kernel_resources.sh,
// profiles/model_set/kernel_resources.txt): the coefficients that k_eval holds in SGPRs are VGPR pairs here.  sgd: 124 (dense) / 127 (strided)
// VGPRs against k_eval<SGD>'s 87 / 73 -- 4 waves per SIMD instead of 5 / 6, no scratch; abc: 64 (dense, 8 waves, k_eval<ABC>: 57) / 70
// (strided: 7 waves, k_eval<ABC>: 61 -- at the hint 8 the strided form kept 32 bytes of scratch).  The dense accesses take their lane
// offset through lane_byte_offset(): with load3_dense_nt the sgd kernel kept 64-bit addresses across the body (48 bytes of scratch at
// 128 VGPRs).
#include "djb_model_hits.inc"                              // row_stride, unit, rows_lds, min_waves, ModelLaunch, stage, model_eval_trip

template <int KIND, int WANT, bool DENSE>
__global__ __launch_bounds__(BLOCK, min_waves(KIND, false)) void k_model_set(Brdf b, const double *rows, int n_mat, int in_lds, long long n, const int32_t *mat,
                                                                             View vi, View vo, View vout)
{
	__shared__ unsigned long long s_exp[256];
	__shared__ double s_pow[384];
	__shared__ double s_atan[KIND == KIND_SGD ? 16 : 1];
	extern __shared__ double s_rows[];                                            // n_mat * STRIDE doubles when in_lds, else none (ModelLaunch)
	const BatchHits<DENSE, true, true> src(n, mat, n_mat);
	b = stage<KIND, KIND == KIND_SGD>(b, s_exp, s_pow, s_atan, s_rows, rows, src.n_mat, in_lds);
	const long long stride = src.stride();
	for (long long j0 = src.start(); j0 < src.count(); j0 += stride)                      // j0: workgroup-uniform
		model_eval_trip<KIND, WANT>(src, j0, s_rows, b, rows, in_lds, vi, vo, vout);
}

template <int KIND, int WANT>
hipError_t launch_set(hipStream_t s, const double *rows, int n_mat, bool rows_global, long long n, const int32_t *mat, const View &i, const View &o,
                      const View &out)
{
	const ModelLaunch L(KIND, n_mat, rows_global, false);
	dim3 g(djbk::grid_capped(n, BLOCK, GRID_CAP)), t(BLOCK);
	if (djbk::dense_strict(i) && djbk::dense_strict(o) && djbk::dense_strict(out))
		hipLaunchKernelGGL((k_model_set<KIND, WANT, true>), g, t, L.lds, s, L.b, rows, n_mat, L.in_lds, n, mat, i, o, out);
	else
		hipLaunchKernelGGL((k_model_set<KIND, WANT, false>), g, t, L.lds, s, L.b, rows, n_mat, L.in_lds, n, mat, i, o, out);
	return hipGetLastError();
}

} // namespace

namespace djbk {

int model_set_row_stride(int kind) { return row_stride(kind); }

hipError_t launch_model_set_eval(hipStream_t s, int kind, const double *rows, int n_mat, bool rows_global, long long n, const int32_t *material,
                                 const View &i, const View &o, const View &out, bool want_cos)
{
	if (n <= 0) return hipSuccess;
	if (kind == KIND_SGD)
		return want_cos ? launch_set<KIND_SGD, 2>(s, rows, n_mat, rows_global, n, material, i, o, out)
		                : launch_set<KIND_SGD, 1>(s, rows, n_mat, rows_global, n, material, i, o, out);
	if (kind == KIND_ABC)
		return want_cos ? launch_set<KIND_ABC, 2>(s, rows, n_mat, rows_global, n, material, i, o, out)
		                : launch_set<KIND_ABC, 1>(s, rows, n_mat, rows_global, n, material, i, o, out);
	return hipErrorInvalidValue;
}

} // namespace djbk
