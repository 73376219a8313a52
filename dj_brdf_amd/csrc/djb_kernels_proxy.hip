// djb_kernels_proxy.hip -- proxy importance sampling, the per-bounce step of the dj_merl / dj_utia / dj_sgd / dj_abc plugins in one launch:
//     i      = proxy.sample(u1, u2, o, proxy_params)           microfacet::sample, dj_brdf.h:1669-1700
//     pdf    = proxy.pdf(i, o, proxy_params)                   microfacet::pdf,    dj_brdf.h:1713-1730 (dot(i, h), no sat)
//     weight = target.evalp(i, o) / pdf                        vec3 / float = (1.0f / pdf) * v, dj_brdf.h:601
// with weight = 0 and pdf = 0 where i.z <= 0 (the plugins' side check; a NaN i.z does not take it).  The three parts are the per-unit
// code the separate operators run (mf_sample, the pdf arm of mf_eval_pdf, eval_one), so every float is the one the three-call route
// produces; what is saved is the traffic -- 48 B per unit instead of 124 -- and two launches.  Nothing is carried over from the sampler
// into the pdf: the reference normalises i + o again (a different h than the sampler's, bit-wise), and its sigma(o) is
// sqrt / reciprocal where the sampler's stretched view direction is an inverse square root -- different operation sequences,
// different floats.  The compiler shares what really is the same (the stretched components a, bb, c of o).
//
// Proxy kinds: ggx, beckmann (the general per-lane sampler, as k_sample_pp), tabular, tabular_anisotropic.  Target kinds: merl, utia,
// sgd, abc.  MERL: tier 1 (merl_index_fast) decides the bin of nearly every pair; a pair it declines waits -- with its pdf, its
// direction already stored -- in a per-wave LDS queue and is finished by the exact index (merl_index) in dense waves, as in
// k_merl_fast.  The other targets run eval_one in place, sgd / abc with their decided fast tier as in k_eval.
#include "djb_internal.hpp"
#include "djb_worklist.hpp"

using namespace djbdev;

namespace {

// tabular_anisotropic as the proxy: its four elev x azim grids (qf2 for the sampler, sigma and p22 for the pdf; 2 x 32 KB + 32 KB at
// 90 x 90) are staged in LDS once per workgroup, so the workgroup is large (as k_eval's); 512 with a MERL target, whose queues take
// 4.5 KB per wave
constexpr int proxy_block(int pkind, int tkind) { return pkind == KIND_TABULAR_ANISO ? (tkind == KIND_MERL ? 512 : 1024) : 256; }
// floats of table staging: what k_sample stages for the kind (qf | qf2 grid + qf1) plus what k_eval stages (p22 + sigma | both grids)
constexpr int proxy_tab_lds(int pkind) { return pkind == KIND_TABULAR ? 2048 + 3072 : pkind == KIND_TABULAR_ANISO ? 8192 + 1024 + 16384 + 768 : 0; }

// the queue of the pairs MERL's tier 1 declines, 9 words per record: {k lo, k hi, i.xyz, o.xyz, pdf}.  It is the extra-trip record queue of
// djb_worklist.hpp written out: through recq_push / recq_drain the eight MERL-target instantiations took 2 more VGPRs each (63 -> 65,
// 65 -> 67, 67 -> 69: the lane's slot address hoisted out of the batch loop, the pdf word read before merl_index instead of after it),
// and the form of the drain that reads the record in place moved the code of every other kernel that uses the helper
// (profiles/wave_queue/proxy_trial.txt).  The five other kernels use the helper; this one keeps its own copy until a form exists that costs nothing.

template <int PKIND, int TKIND, bool DENSE>
__global__ __launch_bounds__(proxy_block(PKIND, TKIND)) void k_evalp_is_proxy(Brdf pb, Params pp, Brdf tb, Params tp, long long n,
                                                                             const float *u1a, const float *u2a, View vo, View vw_out,
                                                                             View vi_out, float *out_pdf, MerlGuard g, int merl_exact)
{
	constexpr int BS = proxy_block(PKIND, TKIND);
	constexpr bool MERLQ = TKIND == KIND_MERL;
	// ---- staging: the union of what k_sample and k_eval stage for the proxy kind and k_eval for the target kind
	constexpr bool GLIBCT = PKIND == KIND_BECKMANN;                                       // logf / expf / powf of Beckmann's quantile functions
	constexpr bool EXPT = PKIND == KIND_BECKMANN || TKIND == KIND_SGD || TKIND == KIND_ABC, POWT = TKIND == KIND_SGD || TKIND == KIND_ABC;
	constexpr bool ATANT = PKIND == KIND_TABULAR || PKIND == KIND_TABULAR_ANISO || TKIND == KIND_SGD;
	__shared__ double s_glibc[GLIBCT ? GLIBC_LDS_WORDS : 1];
	__shared__ unsigned long long s_exp[EXPT ? 256 : 1];
	__shared__ double s_pow[POWT ? 384 : 1];
	__shared__ double s_atan[ATANT ? 16 : 1];
	__shared__ unsigned int s_q[MERLQ ? BS / 64 : 1][9][MERLQ ? RECQ_CAP : 1];
	GlibcTabs gt = glibc_tabs_global();
	if (GLIBCT) gt = glibc_tabs_to_lds(s_glibc, threadIdx.x, BS);
	if (EXPT) { const LdsTab e = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BS); pb.exp_lds = tb.exp_lds = e; if (GLIBCT) gt.exp64 = e; }
	if (POWT) tb.pow_lds = glibc_pow_tab_to_lds(s_pow, threadIdx.x, BS);
	pb.atan_lds = tb.atan_lds = ATANT ? atan_tab_to_lds(s_atan, threadIdx.x) : 0u;
	constexpr int TAB_LDS = proxy_tab_lds(PKIND);
	__shared__ float s_tab[TAB_LDS ? TAB_LDS : 1];
	if (TAB_LDS) {
		int used = 0;
		auto stage = [&](const float *&src, int count) { stage_table<BS>(s_tab, used, src, count); };
		if (PKIND == KIND_TABULAR) { stage(pb.qf, pb.n_qf); stage(pb.p22, pb.n_p22); stage(pb.sigma, pb.n_sigma); }
		if (PKIND == KIND_TABULAR_ANISO) { stage(pb.a_qf2, pb.elev * pb.azim); stage(pb.a_qf1, pb.n_a_qf1); stage(pb.sigma, pb.elev * pb.azim); stage(pb.p22, pb.elev * pb.azim); }
	}
	if (GLIBCT || EXPT || POWT || ATANT || TAB_LDS) __syncthreads();

	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	unsigned int (&q)[9][MERLQ ? RECQ_CAP : 1] = s_q[MERLQ ? wave : 0];
	unsigned int qn = 0;                                                               // wave-uniform
	const long long stride = (long long)gridDim.x * BS;
	for (long long k0 = (long long)blockIdx.x * BS; ; k0 += stride) {                  // k0: workgroup-uniform; MERL: one extra trip flushes the queues
		const bool last = k0 >= n;
		if (!MERLQ && last) break;
		bool amb = false;
		v3 i_ = mk(0, 0, 1), o = mk(0, 0, 1); float pdf = 0.0f;
		const long long k = k0 + t;
		// scalar tile bound, SGPR-base dense accesses (djb_device_units.inc: lane_byte_offset), as in k_sample
		const unsigned int rem = last ? 0u : n - k0 >= (long long)BS ? (unsigned int)BS : (unsigned int)(n - k0);
		if (t < rem) {
			const unsigned int toff = lane_byte_offset(t);
			const float u1 = DENSE ? (*dense_off(u1a + k0, toff)) : u1a[k];
			const float u2 = DENSE ? (*dense_off(u2a + k0, toff)) : u2a[k];
			o = DENSE ? load3_dense_off(vo, k0, toff) : load3(vo, k);
			// ---- proxy: direction, then the pdf-only arm of mf_eval_pdf on (i, o)
			i_ = mf_sample<PKIND>(pb, pp, u1, u2, o, gt);
			const bool side = i_.z <= 0.0f;                                            // false for a NaN i.z: such a sample is evaluated
			v3 w = mk(0, 0, 0);
			if (!side) {
				v3 unused;
				mf_eval_pdf<PKIND, 4>(pb, pp, i_, o, unused, pdf);
				// ---- target: f_r cos at the sampled pair
				if (MERLQ) {
					int idx = 0;
					const bool sure = !merl_exact && merl_index_fast(i_, o, g, idx);
					if (sure) {
						const MerlTexel tx = tb.merl[idx];
						w = divs(scale(i_.z, mk(tx.x, tx.y, tx.z)), pdf);                  // brdf::evalp = eval * i.z, dj_brdf.h:803-806
					} else amb = true;                                                   // the exact index finishes this pair (below)
				} else {
					v3 fr = mk(0, 0, 0); float unused_pdf = 0.0f;
					eval_one<TKIND, 2>(tb, tp, i_, o, fr, unused_pdf);
					w = divs(fr, pdf);
				}
			}
			const unsigned int soff = lane_byte_offset(t);                             // again: the stores sit in another block than the loads
			if (DENSE) { store3_dense_off(vi_out, k0, soff, i_); (*dense_off(out_pdf + k0, soff)) = pdf; }
			else { store3(vi_out, k, i_); out_pdf[k] = pdf; }
			if (!amb) { if (DENSE) store3_dense_off(vw_out, k0, soff, w); else store3(vw_out, k, w); }
		}
		if (MERLQ) {
			const unsigned long long mask = __ballot(amb);
			if (mask) {
				if (amb) {
					const unsigned int j = qn + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
					q[0][j] = (unsigned int)((unsigned long long)k & 0xffffffffull); q[1][j] = (unsigned int)((unsigned long long)k >> 32);
					q[2][j] = __float_as_uint(i_.x); q[3][j] = __float_as_uint(i_.y); q[4][j] = __float_as_uint(i_.z);
					q[5][j] = __float_as_uint(o.x); q[6][j] = __float_as_uint(o.y); q[7][j] = __float_as_uint(o.z);
					q[8][j] = __float_as_uint(pdf);
				}
				qn += (unsigned int)__popcll(mask);
			}
			while (qn >= 64u || (last && qn)) {                                        // a full wave of waiting pairs, or what is left at the end
				const unsigned int cnt = qn < 64u ? qn : 64u;
				qn -= cnt;
				__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
				__builtin_amdgcn_wave_barrier();
				if (lane < cnt) {
					const unsigned int j = qn + lane;
					const long long kq = (long long)(((unsigned long long)q[1][j] << 32) | q[0][j]);
					const v3 iq = mk(__uint_as_float(q[2][j]), __uint_as_float(q[3][j]), __uint_as_float(q[4][j]));
					const v3 oq = mk(__uint_as_float(q[5][j]), __uint_as_float(q[6][j]), __uint_as_float(q[7][j]));
					const MerlTexel tx = tb.merl[merl_index(iq, oq)];
					store3(vw_out, kq, divs(scale(iq.z, mk(tx.x, tx.y, tx.z)), __uint_as_float(q[8][j])));
				}
				__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
				__builtin_amdgcn_wave_barrier();
			}
			if (last) break;
		}
	}
}

template <int PKIND, int TKIND>
hipError_t launch_pair(hipStream_t s, const Brdf &pb, const Params &pp, const Brdf &tb, const Params &tp, long long n, const float *u1,
                       const float *u2, const View &o, const View &out_w, const View &out_i, float *out_pdf, bool merl_exact)
{
	constexpr int BS = proxy_block(PKIND, TKIND);
	const MerlGuard g = MERL_GUARD_DEFAULT;
	dim3 grid(djbk::grid_capped(n, BS, 256LL * 16 * 256 / BS)), block(BS);   // 16 workgroups of 256 per CU's worth, grid-stride beyond
	if (djbk::dense_strict(o) && djbk::dense_strict(out_w) && djbk::dense_strict(out_i))
		hipLaunchKernelGGL((k_evalp_is_proxy<PKIND, TKIND, true>), grid, block, 0, s, pb, pp, tb, tp, n, u1, u2, o, out_w, out_i, out_pdf, g, merl_exact ? 1 : 0);
	else
		hipLaunchKernelGGL((k_evalp_is_proxy<PKIND, TKIND, false>), grid, block, 0, s, pb, pp, tb, tp, n, u1, u2, o, out_w, out_i, out_pdf, g, merl_exact ? 1 : 0);
	return hipGetLastError();
}
template <int PKIND>
hipError_t launch_proxy(hipStream_t s, const Brdf &pb, const Params &pp, const Brdf &tb, const Params &tp, long long n, const float *u1,
                        const float *u2, const View &o, const View &out_w, const View &out_i, float *out_pdf, bool merl_exact)
{
	switch (tb.kind) {
	case KIND_MERL: return launch_pair<PKIND, KIND_MERL>(s, pb, pp, tb, tp, n, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	case KIND_UTIA: return launch_pair<PKIND, KIND_UTIA>(s, pb, pp, tb, tp, n, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	case KIND_SGD: return launch_pair<PKIND, KIND_SGD>(s, pb, pp, tb, tp, n, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	case KIND_ABC: return launch_pair<PKIND, KIND_ABC>(s, pb, pp, tb, tp, n, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	}
	return hipErrorInvalidValue;
}

} // namespace

namespace djbk {

bool evalp_is_proxy_supported(int target_kind, int proxy_kind)
{
	const bool t = target_kind == KIND_MERL || target_kind == KIND_UTIA || target_kind == KIND_SGD || target_kind == KIND_ABC;
	const bool p = proxy_kind == KIND_GGX || proxy_kind == KIND_BECKMANN || proxy_kind == KIND_TABULAR || proxy_kind == KIND_TABULAR_ANISO;
	return t && p;
}

hipError_t launch_evalp_is_proxy(hipStream_t s, const Brdf &target, const Params &tp, const Brdf &proxy, const Params &pp, long long n,
                                 const float *u1, const float *u2, const View &o, const View &out_w, const View &out_i, float *out_pdf,
                                 bool merl_exact)
{
	if (n <= 0) return hipSuccess;
	if (!evalp_is_proxy_supported(target.kind, proxy.kind) || (target.kind == KIND_MERL && target.merl_sparse)) return hipErrorInvalidValue;
	switch (proxy.kind) {
	case KIND_GGX: return launch_proxy<KIND_GGX>(s, proxy, pp, target, tp, n, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	case KIND_BECKMANN: return launch_proxy<KIND_BECKMANN>(s, proxy, pp, target, tp, n, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	case KIND_TABULAR: return launch_proxy<KIND_TABULAR>(s, proxy, pp, target, tp, n, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	case KIND_TABULAR_ANISO: return launch_proxy<KIND_TABULAR_ANISO>(s, proxy, pp, target, tp, n, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
	}
	return hipErrorInvalidValue;
}

} // namespace djbk
