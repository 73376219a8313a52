// djb_kernels_microfacet_set.hip -- microfacet sets: a batch of hits that lands on M resident analytic materials of ONE NDF kind (ggx or
// beckmann), eval / evalp / pdf and sample / evalp_is per hit.
//
// For the single-material kernels (k_eval, k_sample, djb_kernels_eval.hip) the resolved parameters, the Fresnel term and the shadowing
// flag are launch-uniform: kernel arguments, scalar operands.  For the per-pair kernels (k_eval_pp, k_sample_pp) the parameters are
// per-lane, re-derived from a 20-byte record per hit (params_from_pdfparams: the square root of 1 - rho^2, the normal's normalisation and
// no reciprocals, so mf_p22 takes its three IEEE divisions), while Fresnel term and flag stay those of one object.  Here all three move
// with the hit's id: one ROW per material (djb_microfacet_row.hpp: MfRow, 88 bytes), resolved once on the host exactly as the
// single-material call resolves its djb_params -- r_ax / r_t2 included -- and read per lane.
//   k_mf_set<KIND, WANT, FRK, DENSE>         one hit per lane over BatchHits; eval_one<KIND, WANT, FRK> -- the function k_eval and (through
//                                            pp_one) k_eval_pp call -- on a lane-private Params and a lane-private Brdf whose fr / shadow
//                                            are the hit's row
//   k_mf_set_sample<KIND, IS, FRK, DENSE>    sample_one<KIND, IS, FRK>, the function k_sample and k_sample_pp call, likewise: Beckmann's
//                                            one Newton inversion per lane (the general path, as k_sample_pp; the two-path sampler of
//                                            djb_kernels_sample.hip needs wave-uniform parameters)
// so an active hit has the bits of the single-material call.
//
// The path was read for launch-uniform assumptions.  What was found:
//   b.shadow       mf_eval_pdf / mf_evalp_is_tail branch on it (`if (b.shadow) g1i = ...`) and mf_gaf_from_g1 selects on it: plain C++ on a
//                  struct member, now a VGPR; a wave that mixes flags runs the sigma(i) side under EXEC for the lanes that have it.
//                  Nothing reads the flag through a scalar path (no readfirstlane, no "s" constraint).
//   STD            the standard-frame variants (eval_one<..., true>) leave out the terms a launch-uniform test found to be zero.  Not
//                  used here: a set mixes frames, and the test would be per lane.  Every hit takes the general form, which gives the
//                  same floats (djb_device_microfacet.inc says why), so the bits do not depend on which one the single-material call took.
//   fdiv_r         float(double(a) * R) with the row's R in a VGPR pair instead of an SGPR pair; `R != 0.0` becomes a per-lane test (a
//                  row whose ax or t2 is 0 / NaN carries R = 0 and divides).  Its correctness argument is per operand pair.
//   unpolarized    fresnel_eval / fresnel_eval_k test a[0] == a[1] == a[2] to evaluate one channel for three: per lane here, both sides
//                  give the same value for such a row (the same function of the same arguments).
//   fma_sk         "only for literals (an s operand that is not uniform would be read from one lane)": every call site on this path
//                  passes a literal addend; no row value reaches one.
//   staged tables  exp_lds (Beckmann's fp64 exp) and the GlibcTabs of its quantile functions are libm tables, the same for every row;
//                  pow_lds / atan_lds are not on this path (glibc_pow of the sgd Fresnel term's cold branch reads the global copy, as it
//                  does in k_eval<GGX, ., -1>).
//   beckmann_qf2_radial's opaque trip bound (asm "+s") holds the literal 10.
//   The sharp-lobe kernel k_eval_bk_sharp and the two-path sampler k_sample_bk are launch decisions on uniform parameters; both are
//   bit-identical to eval_one / sample_one by their own tests, and neither is used here.
// A translation unit of its own: the code of the existing kernels does not move with this one.
//
// FRK.  The set records at creation whether all rows share one Fresnel kind.  If they do and it is ideal, schlick or unpolarized the
// launch instantiates that kind, as launch_eval_kind does for one object: the fp64 branches of the other terms cost no registers.
// Otherwise (mixed kinds, or all sgd) FRK = -1: fresnel_eval's switch on the row's kind, divergent in a wave that mixes kinds.  pdf alone
// never evaluates the term: the ideal instantiation, as launch_eval_kind.  The same bits either way.
//
// Rows in LDS.  rows = MfRow[M], 88 bytes each = 11 eight-byte units.  Eleven is odd: for ds_read_b64 (banks of 4 bytes, 64 per group of
// 32 lanes) consecutive rows start 22 banks apart and 32 rows cover 32 distinct even banks before the pattern repeats, so the 32 lanes of
// a group that read one field of 32 different rows do so without conflict; for ds_read_b32 (32 banks) 16 rows cover the 16 even banks, a
// 2-way conflict at worst.  An even unit count (96 bytes, say) would fold 32 rows onto 8 banks.  The byte offset id * 88 is below 2^23 at
// DJB_MICROFACET_SET_MAX = 65536: 32-bit offsets.
// When M <= rows_lds(kernel) the workgroup copies the block into dynamic LDS once and every lane reads its row from there; the launch asks
// for M * 88 bytes, so a small set costs no occupancy.  The budget is what the kernel's occupancy -- its VGPR count under the launch
// bounds below, tools/kernel_resources.sh -- leaves of the CU's 160 KiB next to its static tables: rows_lds() and the static_asserts
// below.  Larger sets, and every set under DJB_OPT_MICROFACET_SET_ROWS_GLOBAL, read their rows from global memory with the base in SGPRs
// and the 32-bit byte offset in a VGPR (L2 resident: 5.5 MiB at the maximal M).  The switch is a kernel argument: workgroup-uniform.  Only
// the loads are written twice (one address space each); the row lands in registers and the body follows once.
// Grid: rows in LDS -- a persistent grid of at most GRID_CAP workgroups, so the copy is paid once per resident workgroup and not once per
// 256 hits; rows in global memory -- one workgroup per 256 hits, which is what k_eval / k_sample measured best for these two lobes.
//
// A hit whose id is outside [0, M) is inactive, as is a lane past the end of the batch: +0.0f in every output of the call (nothing, past
// the end), no address formed from its id, no row read; a wave without an active lane skips the arithmetic.  Every lane reads its hit
// before it writes it: index-aligned in-place calls are supported.  Streams are non-temporal where dense, each touched once:
// eval + pdf 4 (id) + 24 + 16 = 44 B per hit, evalp_is 4 + 8 + 12 + 28 = 52 B, sample 4 + 8 + 12 + 12 = 36 B.
#include "djb_internal.hpp"
#include <string.h>

using namespace djbdev;

namespace {

constexpr int BLOCK = 256;
constexpr long long GRID_CAP = 256LL * 8;                  // 256 CUs x the 8 workgroups a CU holds at most: every resident slot, one copy each

#include "djb_hit_source.inc"                              // BatchHits

// Occupancy and the LDS budget.  Registers (tools/kernel_resources.sh, profiles/microfacet_set/kernel_resources.txt): the row's 22 dwords
// are VGPRs where k_eval holds SGPRs, and the non-temporal dense streams through lane_byte_offset() keep the addresses out of the body.
//   ggx       eval 38 - 60 VGPRs, sample / evalp_is 32 - 56: 8 waves per SIMD throughout (k_eval<GGX> 24 - 60, k_eval_pp<GGX> 38 - 63)
//   beckmann  eval 58 - 74, sample / evalp_is 40 - 68: 8 waves for the forms with a compile-time Fresnel kind but the strided fused ones
//             (66: 7 waves), 7 for the FRK = -1 forms, 6 for the strided fused FRK = -1 pair (74) (k_eval<BECKMANN> 44 - 63,
//             k_eval_pp<BECKMANN> 58 - 75: the same steps)
// No instantiation has scratch.  The launch bound asks for 4 waves, as k_eval does for these lobes; the compiler needs none of the slack.
// At 8 waves per SIMD a CU holds 8 workgroups of 256: each may use 160 KiB / 8 = 20 480 B of LDS before LDS, not registers, limits
// the occupancy.  The largest static part is the Beckmann sampler's: 2048 B of exp table + 768 B of logf / expf / powf tables.  One
// budget for the four kernels: (20 480 - 2 816) / 88 = 200 rows.
constexpr int MF_MIN_WAVES = 4;
constexpr int MF_LDS_PER_WG = 163840 / 8;
constexpr int MF_STATIC_LDS = 2048 + 8 * GLIBC_LDS_WORDS;
constexpr int MF_ROWS_LDS = 200;
constexpr int rows_lds(bool) { return MF_ROWS_LDS; }
static_assert(MF_STATIC_LDS == 2816 && MF_STATIC_LDS + MF_ROWS_LDS * MF_ROW_BYTES <= MF_LDS_PER_WG, "eight workgroups per CU with the rows in LDS");
static_assert(MF_STATIC_LDS + (MF_ROWS_LDS + 1) * MF_ROW_BYTES > MF_LDS_PER_WG, "... and not one row more");
static_assert(MF_ROW_BYTES % 16 == 8, "an odd number of 8-byte units per row (LDS banks, above)");
static_assert(65536ull * MF_ROW_BYTES < (1ull << 31), "the byte offset of the last row fits 32 bits");

// the rows into dynamic LDS, as 8-byte units (the caller's barrier follows)
DJB_DEV void stage_rows(double *s_rows, const MfRow *rows, unsigned int n_mat)
{
	const double *src = (const double *)rows;
	const unsigned int count = n_mat * (unsigned int)(MF_ROW_BYTES / 8);
	for (unsigned int j = threadIdx.x; j < count; j += BLOCK) s_rows[j] = src[j];
}
// the hit's row into registers: Params, and the lane's Brdf (the kernel's, with the staged tables) with the row's Fresnel term and flag.
// r points into one address space (the caller's branch)
template <int FRK>
DJB_DEV void take_row(const MfRow *r, Params &p, Brdf &lb)
{
	p = r->p;
	lb.shadow = r->shadow;
	lb.fr.kind = FRK >= 0 ? FRK : r->fr_kind;
	if (FRK != FR_IDEAL) {                                                         // written out: an index that is not a constant keeps the struct in scratch
		lb.fr.a[0] = r->a[0]; lb.fr.a[1] = r->a[1]; lb.fr.a[2] = r->a[2];
		if (FRK < 0) { lb.fr.b[0] = r->b[0]; lb.fr.b[1] = r->b[1]; lb.fr.b[2] = r->b[2]; }      // read by the sgd term alone
	}
}
template <int FRK>
DJB_DEV void row_of(unsigned int id, const double *s_rows, const MfRow *rows, int in_lds, Params &p, Brdf &lb)
{
	const unsigned int off = id * (unsigned int)MF_ROW_BYTES;
	if (in_lds) take_row<FRK>((const MfRow *)((const char *)s_rows + off), p, lb);          // workgroup-uniform: ds_read ...
	else take_row<FRK>((const MfRow *)((const char *)rows + (size_t)off), p, lb);           // ... or uniform base + 32-bit byte offset
}

// ---- eval (WANT 1) / evalp (2) / pdf (4) and the fused 5 / 6 per hit
template <int KIND, int WANT, int FRK, bool DENSE>
__global__ __launch_bounds__(BLOCK, MF_MIN_WAVES) void k_mf_set(Brdf b, const MfRow *rows, int n_mat, int in_lds, long long n, const int32_t *mat, View vi, View vo,
                                                                View vout, float *out_pdf)
{
	__shared__ unsigned long long s_exp[KIND == KIND_BECKMANN ? 256 : 1];
	extern __shared__ double s_rows[];                                            // n_mat * 11 doubles when in_lds, else none
	typedef BatchHits<DENSE, true, true> S;
	const S src(n, mat, n_mat);
	if (KIND == KIND_BECKMANN) b.exp_lds = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
	if (in_lds) stage_rows(s_rows, rows, src.n_mat);
	if (KIND == KIND_BECKMANN || in_lds) __syncthreads();                         // in_lds: workgroup-uniform
	const long long stride = src.stride();
	const unsigned int t = threadIdx.x;
	for (long long j0 = src.start(); j0 < src.count(); j0 += stride) {            // j0: workgroup-uniform
		const bool live = j0 + t < src.count();
		bool act = false;
		unsigned int id = 0u;
		long long k = src.idle(j0, t);
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		if (live) {
			k = src.at(j0, t);
			act = src.id(k, id);
			const typename S::lane_t l = src.lane(j0, t, k);
			i = src.in3(vi, l); o = src.in3(vo, l);
			if (!act) id = 0u;
		}
		v3 fr = mk(0, 0, 0); float pdf = 0.0f;                                    // an inactive hit: +0
		if (__ballot(act) != 0ull) {                                               // wave-uniform: a wave of dead hits computes nothing
			if (act) {
				Params p; Brdf lb = b;
				row_of<FRK>(id, s_rows, rows, in_lds, p, lb);
				eval_one<KIND, WANT, FRK>(lb, p, i, o, fr, pdf);
			}
		}
		if (live) {
			const typename S::lane_t l = src.lane(j0, t, k);                       // again: the stores sit in another block than the loads
			if (WANT & 3) src.out3(vout, l, fr);
			if (WANT & 4) src.out1(out_pdf, l, pdf);
		}
	}
}

// ---- sample (IS false: i alone) / evalp_is (IS true: weight, i, pdf) per hit
template <int KIND, bool IS, int FRK, bool DENSE>
__global__ __launch_bounds__(BLOCK, MF_MIN_WAVES) void k_mf_set_sample(Brdf b, const MfRow *rows, int n_mat, int in_lds, long long n, const int32_t *mat,
                                                                       const float *u1a, const float *u2a, View vo, View vi_out, View vw_out, float *out_pdf)
{
	__shared__ double s_glibc[KIND == KIND_BECKMANN ? GLIBC_LDS_WORDS : 1];       // Beckmann's quantile functions: logf / expf / powf, as k_sample_pp
	__shared__ unsigned long long s_exp[KIND == KIND_BECKMANN ? 256 : 1];
	extern __shared__ double s_rows[];
	typedef BatchHits<DENSE, true, true> S;
	const S src(n, mat, n_mat);
	GlibcTabs gt = glibc_tabs_global();
	if (KIND == KIND_BECKMANN) {
		gt = glibc_tabs_to_lds(s_glibc, threadIdx.x, BLOCK);
		gt.exp64 = b.exp_lds = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
	}
	if (in_lds) stage_rows(s_rows, rows, src.n_mat);
	if (KIND == KIND_BECKMANN || in_lds) __syncthreads();
	const long long stride = src.stride();
	const unsigned int t = threadIdx.x;
	for (long long j0 = src.start(); j0 < src.count(); j0 += stride) {            // j0: workgroup-uniform
		const bool live = j0 + t < src.count();
		bool act = false;
		unsigned int id = 0u;
		long long k = src.idle(j0, t);
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
		v3 w = mk(0, 0, 0), i_ = mk(0, 0, 0); float pdf = 0.0f;                    // an inactive hit: +0 everywhere
		if (__ballot(act) != 0ull) {                                               // wave-uniform
			if (act) {
				Params p; Brdf lb = b;
				row_of<IS ? FRK : FR_IDEAL>(id, s_rows, rows, in_lds, p, lb);       // sample() reads no Fresnel term
				sample_one<KIND, IS, FRK>(lb, p, u1, u2, o, gt, i_, w, pdf);
			}
		}
		if (live) {
			const typename S::lane_t l = src.lane(j0, t, k);
			src.out3(vi_out, l, i_);
			if (IS) { src.out1(out_pdf, l, pdf); src.out3(vw_out, l, w); }
		}
	}
}

// the host side of a launch: whether the rows go to (dynamic) LDS, how much of it, and the grid that goes with either
struct MfLaunch {
	Brdf b; int in_lds; size_t lds; dim3 grid;
	MfLaunch(int kind, int n_mat, bool rows_global, bool sample, long long n)
	{
		memset(&b, 0, sizeof b);                                                   // the kind's Brdf: the kernel adds its staged tables, a lane its row
		b.kind = kind;
		in_lds = !rows_global && n_mat <= rows_lds(sample);
		lds = in_lds ? (size_t)n_mat * MF_ROW_BYTES : 0;
		long long blocks = (n + BLOCK - 1) / BLOCK;
		if (blocks > 0x7fffffffLL) blocks = 0x7fffffffLL;
		grid = dim3((unsigned int)(in_lds ? djbk::grid_capped(n, BLOCK, GRID_CAP) : blocks < 1 ? 1 : blocks));
	}
};

template <int KIND, int FRK>
hipError_t launch_eval_fr(hipStream_t s, const MfRow *rows, int n_mat, bool rows_global, long long n, const int32_t *mat, const View &i, const View &o,
                          const View &out, float *out_pdf, int want)
{
	const MfLaunch L(KIND, n_mat, rows_global, false, n);
	const dim3 t(BLOCK);
	const bool dn = djbk::dense_strict(i) && djbk::dense_strict(o) && djbk::dense_or_null(out);
#define DJB_MF_EVAL(W_) do { if (dn) hipLaunchKernelGGL((k_mf_set<KIND, W_, FRK, true>), L.grid, t, L.lds, s, L.b, rows, n_mat, L.in_lds, n, mat, i, o, out, out_pdf); \
                             else hipLaunchKernelGGL((k_mf_set<KIND, W_, FRK, false>), L.grid, t, L.lds, s, L.b, rows, n_mat, L.in_lds, n, mat, i, o, out, out_pdf); } while (0)
	switch (want) {
	case 1: DJB_MF_EVAL(1); break;
	case 2: DJB_MF_EVAL(2); break;
	case 5: DJB_MF_EVAL(5); break;
	case 6: DJB_MF_EVAL(6); break;
	default: return hipErrorInvalidValue;
	}
#undef DJB_MF_EVAL
	return hipGetLastError();
}
template <int KIND>
hipError_t launch_eval_kind(hipStream_t s, const MfRow *rows, int n_mat, int fr_kind, bool rows_global, long long n, const int32_t *mat, const View &i,
                            const View &o, const View &out, float *out_pdf, int want)
{
	if (want == 4) {                                                               // pdf alone never evaluates the Fresnel term
		const MfLaunch L(KIND, n_mat, rows_global, false, n);
		if (djbk::dense_strict(i) && djbk::dense_strict(o))
			hipLaunchKernelGGL((k_mf_set<KIND, 4, FR_IDEAL, true>), L.grid, dim3(BLOCK), L.lds, s, L.b, rows, n_mat, L.in_lds, n, mat, i, o, out, out_pdf);
		else hipLaunchKernelGGL((k_mf_set<KIND, 4, FR_IDEAL, false>), L.grid, dim3(BLOCK), L.lds, s, L.b, rows, n_mat, L.in_lds, n, mat, i, o, out, out_pdf);
		return hipGetLastError();
	}
	if (fr_kind == FR_IDEAL) return launch_eval_fr<KIND, FR_IDEAL>(s, rows, n_mat, rows_global, n, mat, i, o, out, out_pdf, want);
	if (fr_kind == FR_SCHLICK) return launch_eval_fr<KIND, FR_SCHLICK>(s, rows, n_mat, rows_global, n, mat, i, o, out, out_pdf, want);
	if (fr_kind == FR_UNPOLARIZED) return launch_eval_fr<KIND, FR_UNPOLARIZED>(s, rows, n_mat, rows_global, n, mat, i, o, out, out_pdf, want);
	return launch_eval_fr<KIND, -1>(s, rows, n_mat, rows_global, n, mat, i, o, out, out_pdf, want);
}

template <int KIND>
hipError_t launch_sample_kind(hipStream_t s, const MfRow *rows, int n_mat, int fr_kind, bool rows_global, long long n, const int32_t *mat, const float *u1,
                              const float *u2, const View &o, const View &out_i, const View *out_w, float *out_pdf)
{
	const MfLaunch L(KIND, n_mat, rows_global, true, n);
	const dim3 t(BLOCK);
	const View w = out_w ? *out_w : View{ nullptr, nullptr, nullptr, 0 };
	const bool dn = djbk::dense_strict(o) && djbk::dense_strict(out_i) && djbk::dense_or_null(w);
#define DJB_MF_SAMPLE(IS_, FRK_) do { if (dn) hipLaunchKernelGGL((k_mf_set_sample<KIND, IS_, FRK_, true>), L.grid, t, L.lds, s, L.b, rows, n_mat, L.in_lds, n, mat, u1, u2, o, out_i, w, out_pdf); \
                                      else hipLaunchKernelGGL((k_mf_set_sample<KIND, IS_, FRK_, false>), L.grid, t, L.lds, s, L.b, rows, n_mat, L.in_lds, n, mat, u1, u2, o, out_i, w, out_pdf); \
                                      return hipGetLastError(); } while (0)
	if (!out_w) DJB_MF_SAMPLE(false, -1);
	if (fr_kind == FR_IDEAL) DJB_MF_SAMPLE(true, FR_IDEAL);
	if (fr_kind == FR_SCHLICK) DJB_MF_SAMPLE(true, FR_SCHLICK);
	if (fr_kind == FR_UNPOLARIZED) DJB_MF_SAMPLE(true, FR_UNPOLARIZED);
	DJB_MF_SAMPLE(true, -1);
#undef DJB_MF_SAMPLE
}

} // namespace

namespace djbk {

int microfacet_set_rows_lds() { return MF_ROWS_LDS; }
long long microfacet_set_grid_cap() { return GRID_CAP; }

hipError_t launch_microfacet_set_eval(hipStream_t s, int kind, const MfRow *rows, int n_mat, int fr_kind, bool rows_global, long long n,
                                      const int32_t *material, const View &i, const View &o, const View &out, float *out_pdf, int want)
{
	if (n <= 0) return hipSuccess;
	if (kind == KIND_GGX) return launch_eval_kind<KIND_GGX>(s, rows, n_mat, fr_kind, rows_global, n, material, i, o, out, out_pdf, want);
	if (kind == KIND_BECKMANN) return launch_eval_kind<KIND_BECKMANN>(s, rows, n_mat, fr_kind, rows_global, n, material, i, o, out, out_pdf, want);
	return hipErrorInvalidValue;
}

hipError_t launch_microfacet_set_sample(hipStream_t s, int kind, const MfRow *rows, int n_mat, int fr_kind, bool rows_global, long long n,
                                        const int32_t *material, const float *u1, const float *u2, const View &o, const View &out_i, const View *out_w,
                                        float *out_pdf)
{
	if (n <= 0) return hipSuccess;
	if (kind == KIND_GGX) return launch_sample_kind<KIND_GGX>(s, rows, n_mat, fr_kind, rows_global, n, material, u1, u2, o, out_i, out_w, out_pdf);
	if (kind == KIND_BECKMANN) return launch_sample_kind<KIND_BECKMANN>(s, rows, n_mat, fr_kind, rows_global, n, material, u1, u2, o, out_i, out_w, out_pdf);
	return hipErrorInvalidValue;
}

} // namespace djbk
