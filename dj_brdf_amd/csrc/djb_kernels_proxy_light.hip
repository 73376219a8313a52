// djb_kernels_proxy_light.hip -- the light sample (next-event estimation / MIS) of the dj_merl / dj_utia / dj_sgd / dj_abc plugins in one
// launch, for a GIVEN pair (i, o):
//     fr  = target.evalp(i, o)                                 brdf::evalp, dj_brdf.h:803-806
//     pdf = proxy.pdf(i, o, proxy_params)                      microfacet::pdf, dj_brdf.h:1713-1730 (dot(i, h), no sat)
// with fr = +0 and pdf = +0 where i.z <= 0 || o.z <= 0 (the plugins' guard, mitsuba/dj_merl.cpp:33-42; a NaN z does not take it).
// The other half of the per-bounce step is k_evalp_is_proxy (djb_kernels_proxy.hip); this kernel has its pairs of kinds and its workgroup
// sizes, in a translation unit of its own so that the code of those kernels cannot move; the queue is the shared one of djb_worklist.hpp.  The per-unit functions are the
// ones the separate operators call (the pdf arm of mf_eval_pdf, eval_one, merl_index_fast / merl_index, scale), so every float is the
// one djb_evalp_batch and djb_pdf_batch produce; what is saved is the traffic -- 40 B per pair instead of 64 -- a launch and the
// caller's guard pass.
//
// MERL target: tier 1 (merl_index_fast) decides the bin of nearly every pair; its texel is asked for BEFORE the pdf arithmetic and
// consumed after it (as in k_merl_set_evalp_pdf).  A pair tier 1 declines stores its pdf at once -- the record needs no pdf word -- waits
// in a per-wave LDS queue and is finished by the exact index in dense waves.  A guarded pair reads no table and is never queued.
// Staging: what the PDF side of the proxy and the target's evalp need, no more: none of the sampler's tables (Beckmann's logf / powf
// tables, qf of tabular, qf2 / qf1 of tabular_anisotropic).
#include "djb_internal.hpp"
#include "djb_worklist.hpp"

using namespace djbdev;

namespace {

// the workgroup sizes of k_evalp_is_proxy: tabular_anisotropic stages its sigma and p22 grids (2 x 32 KB at 90 x 90) once per
// workgroup, so the workgroup is large; 512 with a MERL target, whose queues take 4 KB per wave
constexpr int light_block(int pkind, int tkind) { return pkind == KIND_TABULAR_ANISO ? (tkind == KIND_MERL ? 512 : 1024) : 256; }
// floats of table staging: what k_eval stages for the kind (p22 + sigma | both grids)
constexpr int light_tab_lds(int pkind) { return pkind == KIND_TABULAR ? 3072 : pkind == KIND_TABULAR_ANISO ? 16384 : 0; }

constexpr int QW = 8;                                                              // the queue's record: {k lo, k hi, i.xyz, o.xyz}

// DENSE: every view has stride 1 -- the 40 B/pair streams (i, o, fr, pdf) are touched once: non-temporal, so that they leave the L2 to
// the table gathers
template <int PKIND, int TKIND, bool DENSE>
__global__ __launch_bounds__(light_block(PKIND, TKIND)) void k_evalp_pdf_proxy(Brdf pb, Params pp, Brdf tb, Params tp, long long n, View vi, View vo,
                                                                              View vout, float *out_pdf, MerlGuard g, int merl_exact)
{
	constexpr int BS = light_block(PKIND, TKIND);
	constexpr bool MERLQ = TKIND == KIND_MERL;
	constexpr bool OFFS = DENSE && (TKIND == KIND_MERL || TKIND == KIND_UTIA);           // see load3_dense_off_nt
	// ---- staging: what k_eval stages for the proxy kind (the pdf arm) and for the target kind
	constexpr bool EXPT = PKIND == KIND_BECKMANN || TKIND == KIND_SGD || TKIND == KIND_ABC, POWT = TKIND == KIND_SGD || TKIND == KIND_ABC;
	constexpr bool ATANT = PKIND == KIND_TABULAR || PKIND == KIND_TABULAR_ANISO || TKIND == KIND_SGD;
	__shared__ unsigned long long s_exp[EXPT ? 256 : 1];
	__shared__ double s_pow[POWT ? 384 : 1];
	__shared__ double s_atan[ATANT ? 16 : 1];
	__shared__ unsigned int s_q[MERLQ ? BS / 64 : 1][QW][MERLQ ? RECQ_CAP : 1];
	if (EXPT) pb.exp_lds = tb.exp_lds = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BS);
	if (POWT) tb.pow_lds = glibc_pow_tab_to_lds(s_pow, threadIdx.x, BS);
	pb.atan_lds = tb.atan_lds = ATANT ? atan_tab_to_lds(s_atan, threadIdx.x) : 0u;
	constexpr int TAB_LDS = light_tab_lds(PKIND);
	__shared__ float s_tab[TAB_LDS ? TAB_LDS : 1];
	if (TAB_LDS) {
		int used = 0;
		auto stage = [&](const float *&src, int count) { stage_table<BS>(s_tab, used, src, count); };
		if (PKIND == KIND_TABULAR) { stage(pb.p22, pb.n_p22); stage(pb.sigma, pb.n_sigma); }
		if (PKIND == KIND_TABULAR_ANISO) { stage(pb.sigma, pb.elev * pb.azim); stage(pb.p22, pb.elev * pb.azim); }
	}
	if (EXPT || POWT || ATANT || TAB_LDS) __syncthreads();

	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	unsigned int (&q)[QW][MERLQ ? RECQ_CAP : 1] = s_q[MERLQ ? wave : 0];
	unsigned int qn = 0;                                                               // wave-uniform
	const long long stride = (long long)gridDim.x * BS;
	for (long long k0 = (long long)blockIdx.x * BS; ; k0 += stride) {                  // k0: workgroup-uniform; MERL: one extra trip flushes the queues
		const bool last = k0 >= n;
		if (!MERLQ && last) break;
		bool amb = false;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		const long long k = k0 + t;
		const unsigned int rem = last ? 0u : n - k0 >= (long long)BS ? (unsigned int)BS : (unsigned int)(n - k0);   // scalar tile bound
		if (t < rem) {
			const unsigned int toff = OFFS ? lane_byte_offset(t) : 0u;
			i = !DENSE ? load3(vi, k) : OFFS ? load3_dense_off_nt(vi, k0, toff) : load3_dense_nt(vi, k0, t);
			o = !DENSE ? load3(vo, k) : OFFS ? load3_dense_off_nt(vo, k0, toff) : load3_dense_nt(vo, k0, t);
			v3 fr = mk(0, 0, 0); float pdf = 0.0f;                                     // below the horizon: +0, nothing read
			if (!(i.z <= 0.0f || o.z <= 0.0f)) {                                       // dj_merl.cpp:33-42; a NaN z is evaluated
				v3 unused;
				if (MERLQ) {
					int idx = 0;
					const bool decided = !merl_exact && merl_index_fast(i, o, g, idx);
					MerlTexel tx = { 0.0f, 0.0f, 0.0f };
					if (decided) tx = tb.merl[idx];                                      // in flight across the pdf
					mf_eval_pdf<PKIND, 4>(pb, pp, i, o, unused, pdf);                    // microfacet::pdf
					if (decided) fr = scale(i.z, mk(tx.x, tx.y, tx.z));                  // brdf::evalp = eval * i.z
					else amb = true;                                                     // the exact index finishes this pair (below)
				} else {
					float unused_pdf = 0.0f;
					mf_eval_pdf<PKIND, 4>(pb, pp, i, o, unused, pdf);
					eval_one<TKIND, 2>(tb, tp, i, o, fr, unused_pdf);
				}
			}
			const unsigned int soff = OFFS ? lane_byte_offset(t) : t << 2;             // again: the stores sit in another block than the loads
			if (DENSE) __builtin_nontemporal_store(pdf, dense_off(out_pdf + k0, soff)); else __builtin_nontemporal_store(pdf, out_pdf + k);
			if (!amb) { if (!DENSE) store3(vout, k, fr); else if (OFFS) store3_dense_off_nt(vout, k0, soff, fr); else store3_dense_nt(vout, k0, t, fr); }
		}
		if (MERLQ) {
			unsigned int rec[QW];                                                      // built here, outside the branches above (djb_worklist.hpp)
			rec_put_k(rec, k); rec_put_v3(rec, 2, i); rec_put_v3(rec, 5, o);
			recq_push(q, qn, lane, amb, rec);
			recq_drain(q, qn, lane, last, [&](const unsigned int *r) {
				const v3 iq = rec_v3(r, 2);
				const MerlTexel tx = tb.merl[merl_index(iq, rec_v3(r, 5))];
				store3(vout, rec_k(r), scale(iq.z, mk(tx.x, tx.y, tx.z)));
			});
			if (last) break;
		}
	}
}

template <int PKIND, int TKIND>
hipError_t launch_pair(hipStream_t s, const Brdf &pb, const Params &pp, const Brdf &tb, const Params &tp, long long n, const View &i, const View &o,
                       const View &out_fr, float *out_pdf, bool merl_exact)
{
	constexpr int BS = light_block(PKIND, TKIND);
	const MerlGuard g = MERL_GUARD_DEFAULT;
	dim3 grid(djbk::grid_capped(n, BS, 256LL * 16 * 256 / BS)), block(BS);   // 16 workgroups of 256 per CU's worth, grid-stride beyond
	if (djbk::dense_strict(i) && djbk::dense_strict(o) && djbk::dense_strict(out_fr))
		hipLaunchKernelGGL((k_evalp_pdf_proxy<PKIND, TKIND, true>), grid, block, 0, s, pb, pp, tb, tp, n, i, o, out_fr, out_pdf, g, merl_exact ? 1 : 0);
	else
		hipLaunchKernelGGL((k_evalp_pdf_proxy<PKIND, TKIND, false>), grid, block, 0, s, pb, pp, tb, tp, n, i, o, out_fr, out_pdf, g, merl_exact ? 1 : 0);
	return hipGetLastError();
}
template <int PKIND>
hipError_t launch_proxy(hipStream_t s, const Brdf &pb, const Params &pp, const Brdf &tb, const Params &tp, long long n, const View &i, const View &o,
                        const View &out_fr, float *out_pdf, bool merl_exact)
{
	switch (tb.kind) {
	case KIND_MERL: return launch_pair<PKIND, KIND_MERL>(s, pb, pp, tb, tp, n, i, o, out_fr, out_pdf, merl_exact);
	case KIND_UTIA: return launch_pair<PKIND, KIND_UTIA>(s, pb, pp, tb, tp, n, i, o, out_fr, out_pdf, merl_exact);
	case KIND_SGD: return launch_pair<PKIND, KIND_SGD>(s, pb, pp, tb, tp, n, i, o, out_fr, out_pdf, merl_exact);
	case KIND_ABC: return launch_pair<PKIND, KIND_ABC>(s, pb, pp, tb, tp, n, i, o, out_fr, out_pdf, merl_exact);
	}
	return hipErrorInvalidValue;
}

} // namespace

namespace djbk {

hipError_t launch_evalp_pdf_proxy(hipStream_t s, const Brdf &target, const Params &tp, const Brdf &proxy, const Params &pp, long long n,
                                  const View &i, const View &o, const View &out_fr, float *out_pdf, bool merl_exact)
{
	if (n <= 0) return hipSuccess;
	if (!evalp_is_proxy_supported(target.kind, proxy.kind) || (target.kind == KIND_MERL && target.merl_sparse)) return hipErrorInvalidValue;
	switch (proxy.kind) {
	case KIND_GGX: return launch_proxy<KIND_GGX>(s, proxy, pp, target, tp, n, i, o, out_fr, out_pdf, merl_exact);
	case KIND_BECKMANN: return launch_proxy<KIND_BECKMANN>(s, proxy, pp, target, tp, n, i, o, out_fr, out_pdf, merl_exact);
	case KIND_TABULAR: return launch_proxy<KIND_TABULAR>(s, proxy, pp, target, tp, n, i, o, out_fr, out_pdf, merl_exact);
	case KIND_TABULAR_ANISO: return launch_proxy<KIND_TABULAR_ANISO>(s, proxy, pp, target, tp, n, i, o, out_fr, out_pdf, merl_exact);
	}
	return hipErrorInvalidValue;
}

} // namespace djbk
