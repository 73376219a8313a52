// djb_kernels_scene_proxy.hip -- scenes: the two per-hit proxy steps of a path vertex on a batch that lands on MERL, UTIA, sgd and abc
// materials at once (the eval / evalp half: djb_kernels_scene.hip):
//   sampling       i = proxy.sample(u1, u2, o), pdf = proxy.pdf(i, o), weight = material.evalp(i, o) / pdf; i stored, weight 0 and pdf 0 where i.z <= 0
//   light sample   fr = material.evalp(i, o), pdf = proxy.pdf(i, o) of a GIVEN pair; both +0 where i.z <= 0 || o.z <= 0
// (a NaN z takes neither test).  The shape is that of the eval call: the batch is partitioned by kind on the device -- k_scene_count and
// k_scene_scan of djb_kernels_scene.hip, unchanged, through launch_scene_count_scan, then
//   k_scene_scatter_proxy<LIGHT>     k_scene_scatter with the +0 of an inactive hit stored in EVERY output of the call (7 floats / 4 floats)
// and one kernel per member set the scene has runs on its dense list of hit indices.  No kernel dispatches on kind per lane:
//   k_scene_merl_is<PKIND>           k_evalp_is_proxy_merl_set's body (djb_kernels_merl_set.hip): Params[id] per lane, tier 1 in place, the
//   k_scene_merl_light<PKIND>        10-word record queue and the extra trip / k_merl_set_evalp_pdf's body: Params[id] asked for before the
//                                    texel, the texel in flight across the pdf, the 9-word record queue
//   k_scene_utia_is<PKIND>           k_evalp_is_proxy<PKIND, KIND_UTIA> / k_evalp_pdf_proxy<PKIND, KIND_UTIA> (djb_kernels_proxy.hip,
//   k_scene_utia_light<PKIND>        djb_kernels_proxy_light.hip) per hit: the hit's Params from the utia set's block, eval_one<KIND_UTIA, 2> in
//                                    place on a lane-private Brdf whose `utia` is the hit's table (what k_scene_utia_fix binds).  No
//                                    worklist, no fix pass
//   k_scene_model_is<KIND>           k_model_set_evalp_is_proxy's / k_model_set_evalp_pdf's body (djb_kernels_model_set_proxy.hip): unit<KIND, 2>,
//   k_scene_model_light<KIND>        rows in dynamic LDS or global memory, the proxy tables per lane from the set's resident block
// PKIND: ggx or beckmann, the lobe of the merl and utia parts.  The loop of every per-kind kernel runs over list positions j below
// count[kind] (a scalar load, workgroup-uniform), k = list[offset + j]; every gather and scatter goes through k.  The grid is sized for the
// chunk, an upper bound, with the member kernel's cap: a workgroup beyond the count leaves before it stages anything.  The per-unit
// functions are the ones the member kernels call, so an active hit has the bits of its member's call.  The MERL bodies and the sgd / abc
// sampling body exist once, over a hit source (djb_merl_hits.inc, djb_model_hits.inc; here ListHits, djb_scene_part.inc); the sgd / abc
// light sample and the utia kernels are written out.
//
// UTIA, the indices of the exact path for ANY sampled direction (utia_prepare<false>, djb_device_tables.inc; the sampler may return NaN
// components): a NaN azimuth makes the pair `dead` and replaces all four angles by 1; a polar angle that is NaN compares false with
// every bound, so utia_bin15 (djb_device.hpp, the device form: a sum of four comparisons) gives 0, and one >= 90 is `dead`: both polar
// cells lie in [0, 4], the second theta_i cell in [1, 5]; an azimuth leaves the wrap loops in [0, 360) and utia_bin7p5 corrects its
// estimate into [0, 47].  The record index is at most 288 * (48 * 5 + 47) + 48 * 4 + 47 = 82 895 < 288 * 288, and six float4 of an
// eight-float4 record are read: an active hit never addresses outside its own material's 288 * 288 * 8 float4.
//
// Nothing is read back to the host and there are no atomics.  Every lane reads its hit before it writes it, kinds touch disjoint hits,
// the drains of the MERL queues work on their records alone and no kernel takes a second pass over a hit: index-aligned in-place views
// are supported.  Hit indices are chunk-relative and 32 bits wide (the host runs chunks of at most 2^26 hits, djb_scene.hip).
// Bytes per active hit, counted from the signatures (not measured): the per-kind kernel moves what its member's kernel moves -- sampling
// 4 (id) + 4 + 4 + 12 read, 12 + 12 + 4 written = 52; light sample 4 + 12 + 12 read, 12 + 4 written = 44 -- plus 4 of list read; the
// partition reads the id twice and writes 4 of list: 68 and 60 in all, the slot table (L2 resident) aside.
#include "djb_internal.hpp"
#include "djb_worklist.hpp"
#include <string.h>

using namespace djbdev;

namespace {

#include "djb_scene_part.inc"                              // BLOCK, TILE, K_*, Hits, slot_of, kind_of, local_of, ListHits, wave_tile, scatter_hits
constexpr long long GRID_CAP = 256LL * 16;                 // as every member kernel: k_evalp_is_proxy_merl_set, k_evalp_is_proxy (256-thread workgroups), k_model_set_evalp_is_proxy
static_assert(GRID_CAP * BLOCK == djbk::SCENE_PROXY_TRIP, "the trip size the tests restate");

#include "djb_merl_hits.inc"                               // merl_set_texel, the queue record, merl_is_hits / merl_light_hits
#include "djb_utia_hits.inc"                               // TABLE_F4, utia_target
#include "djb_model_hits.inc"                              // row_stride, unit, rows_lds, min_waves, ModelLaunch, proxy_of, model_is_trip

// ---- the partition's third step: the list, and +0 in every output of an inactive hit.  LIGHT: va = out_fr; else va = out_weight, vb = out_i
template <bool LIGHT>
__global__ __launch_bounds__(BLOCK) void k_scene_scatter_proxy(const unsigned int *slots, unsigned int n_slots, unsigned int m, const int32_t *mat,
                                                               unsigned int n_tiles, const unsigned int *tiles, unsigned int *list, View va, View vb,
                                                               float *out_pdf)
{
	scatter_hits(slots, n_slots, m, mat, n_tiles, tiles, list, [&](unsigned int k) {
		store3(va, (long long)k, mk(0, 0, 0));
		if (!LIGHT) store3(vb, (long long)k, mk(0, 0, 0));
		out_pdf[k] = 0.0f;
	});
}

// ---- merl: merl_is_hits / merl_light_hits over the list
template <int PKIND>
__global__ __launch_bounds__(BLOCK) void k_scene_merl_is(Hits h, Brdf pb, const Params *params, const MerlTexel *tex, unsigned int n_mat,
                                                         const float *u1a, const float *u2a, View vo, View vw_out, View vi_out, float *out_pdf,
                                                         MerlGuard g, int merl_exact)
{
	constexpr bool GLIBCT = PKIND == KIND_BECKMANN;
	__shared__ double s_glibc[GLIBCT ? GLIBC_LDS_WORDS : 1];
	__shared__ unsigned long long s_exp[GLIBCT ? 256 : 1];
	__shared__ unsigned int s_q[BLOCK / 64][10][RECQ_CAP];
	merl_is_hits<PKIND>(ListHits(h, K_MERL, n_mat), s_glibc, s_exp, s_q, pb, params, tex, u1a, u2a, vo, vw_out, vi_out, out_pdf, g, merl_exact);
}

template <int PKIND>
__global__ __launch_bounds__(BLOCK) void k_scene_merl_light(Hits h, Brdf pb, const Params *params, const MerlTexel *tex, unsigned int n_mat, View vi,
                                                            View vo, View vout, float *out_pdf, MerlGuard g, int merl_exact)
{
	__shared__ unsigned long long s_exp[PKIND == KIND_BECKMANN ? 256 : 1];
	__shared__ unsigned int s_q[BLOCK / 64][9][RECQ_CAP];
	merl_light_hits<PKIND>(ListHits(h, K_MERL, n_mat), s_exp, s_q, pb, params, tex, vi, vo, vout, out_pdf, g, merl_exact);
}

// ---- utia: the single-material proxy kernels per hit.  tb: kind utia, nothing else set; its `utia` becomes the hit's table per lane
template <int PKIND>
__global__ __launch_bounds__(BLOCK) void k_scene_utia_is(Hits h, Brdf pb, Brdf tb, const Params *params, const float4 *tab, unsigned int n_mat,
                                                         const float *u1a, const float *u2a, View vo, View vw_out, View vi_out, float *out_pdf)
{
	static_assert(PKIND == KIND_GGX || PKIND == KIND_BECKMANN, "the proxy of a UTIA member is an analytic lobe");
	constexpr bool GLIBCT = PKIND == KIND_BECKMANN;
	__shared__ double s_glibc[GLIBCT ? GLIBC_LDS_WORDS : 1];
	__shared__ unsigned long long s_exp[GLIBCT ? 256 : 1];
	const unsigned int cnt = h.hdr[K_UTIA], first = h.hdr[4 + K_UTIA];
	if (blockIdx.x * (unsigned int)BLOCK >= cnt) return;                           // workgroup-uniform, before the staging and its barrier
	GlibcTabs gt = glibc_tabs_global();
	if (GLIBCT) {
		gt = glibc_tabs_to_lds(s_glibc, threadIdx.x, BLOCK);
		const LdsTab e = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
		pb.exp_lds = tb.exp_lds = e; gt.exp64 = e;
		__syncthreads();
	}
	pb.atan_lds = tb.atan_lds = 0u;
	const Params none = {};
	const unsigned int stride = gridDim.x * (unsigned int)BLOCK;
	for (unsigned int j = blockIdx.x * (unsigned int)BLOCK + threadIdx.x; j < cnt; j += stride) {
		const unsigned int k = h.list[first + j];
		unsigned int id;
		v3 w = mk(0, 0, 0), i_ = mk(0, 0, 0); float pdf = 0.0f;
		if (local_of(h, k, K_UTIA, n_mat, id)) {
			const float u1 = u1a[k], u2 = u2a[k];
			const v3 o = load3(vo, (long long)k);
			const Params pp = params[id];
			i_ = mf_sample<PKIND>(pb, pp, u1, u2, o, gt);
			if (!(i_.z <= 0.0f)) {                                                      // the side check; a NaN i.z is evaluated
				v3 unused, fr = mk(0, 0, 0); float unused_pdf = 0.0f;
				mf_eval_pdf<PKIND, 4>(pb, pp, i_, o, unused, pdf);
				tb.utia = tab + (size_t)id * (size_t)TABLE_F4;
				eval_one<KIND_UTIA, 2>(tb, none, i_, o, fr, unused_pdf);                // indices clamped for any i_, o: the file's head
				w = divs(fr, pdf);
			}
		}
		store3(vi_out, (long long)k, i_); out_pdf[k] = pdf; store3(vw_out, (long long)k, w);
	}
}

template <int PKIND>
__global__ __launch_bounds__(BLOCK) void k_scene_utia_light(Hits h, Brdf pb, Brdf tb, const Params *params, const float4 *tab, unsigned int n_mat,
                                                            View vi, View vo, View vout, float *out_pdf)
{
	static_assert(PKIND == KIND_GGX || PKIND == KIND_BECKMANN, "the proxy of a UTIA member is an analytic lobe");
	constexpr bool EXPT = PKIND == KIND_BECKMANN;
	__shared__ unsigned long long s_exp[EXPT ? 256 : 1];
	const unsigned int cnt = h.hdr[K_UTIA], first = h.hdr[4 + K_UTIA];
	if (blockIdx.x * (unsigned int)BLOCK >= cnt) return;
	if (EXPT) {
		pb.exp_lds = tb.exp_lds = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
		__syncthreads();
	}
	pb.atan_lds = tb.atan_lds = 0u;
	const Params none = {};
	const unsigned int stride = gridDim.x * (unsigned int)BLOCK;
	for (unsigned int j = blockIdx.x * (unsigned int)BLOCK + threadIdx.x; j < cnt; j += stride) {
		const unsigned int k = h.list[first + j];
		unsigned int id;
		const bool act = local_of(h, k, K_UTIA, n_mat, id);
		const v3 i = load3(vi, (long long)k), o = load3(vo, (long long)k);
		v3 fr = mk(0, 0, 0); float pdf = 0.0f;                                         // below the horizon: +0, nothing read
		if (act && !(i.z <= 0.0f || o.z <= 0.0f)) {                                    // the plugins' guard; a NaN z is evaluated
			v3 unused; float unused_pdf = 0.0f;
			mf_eval_pdf<PKIND, 4>(pb, params[id], i, o, unused, pdf);
			tb.utia = tab + (size_t)id * (size_t)TABLE_F4;
			eval_one<KIND_UTIA, 2>(tb, none, i, o, fr, unused_pdf);
		}
		out_pdf[k] = pdf; store3(vout, (long long)k, fr);
	}
}

// ---- sgd / abc: model_is_trip over the list; the light sample written out
template <int KIND>
__global__ __launch_bounds__(BLOCK, min_waves(KIND, true)) void k_scene_model_is(Hits h, Brdf b, Params pp, ModelSetProxy px, const double *rows, unsigned int n_mat,
                                                                                 int in_lds, const float *u1a, const float *u2a, View vo, View vw_out,
                                                                                 View vi_out, float *out_pdf)
{
	__shared__ unsigned long long s_exp[256];
	__shared__ double s_pow[384];
	__shared__ double s_atan[16];
	extern __shared__ double s_rows[];                                            // n_mat * STRIDE doubles when in_lds, else none
	const ListHits src(h, KIND == KIND_SGD ? K_SGD : K_ABC, n_mat);
	if (src.none()) return;                                                        // workgroup-uniform, before the staging and its barrier
	b = stage<KIND, true>(b, s_exp, s_pow, s_atan, s_rows, rows, src.n_mat, in_lds);
	const unsigned int stride = src.stride();
	for (unsigned int j0 = src.start(); j0 < src.count(); j0 += stride)                      // j0: workgroup-uniform
		model_is_trip<KIND>(src, j0, s_rows, b, pp, px, rows, in_lds, u1a, u2a, vo, vw_out, vi_out, out_pdf);
}

// k_model_set_evalp_pdf over the list, written out: on one body the pair did not keep its instructions
template <int KIND>
__global__ __launch_bounds__(BLOCK, min_waves(KIND, true)) void k_scene_model_light(Hits h, Brdf b, Params pp, ModelSetProxy px, const double *rows,
                                                                              unsigned int n_mat, int in_lds, View vi, View vo, View vout, float *out_pdf)
{
	constexpr unsigned int STRIDE = (unsigned int)row_stride(KIND);
	constexpr unsigned int Q = KIND == KIND_SGD ? K_SGD : K_ABC;
	__shared__ unsigned long long s_exp[256];
	__shared__ double s_pow[384];
	__shared__ double s_atan[16];
	extern __shared__ double s_rows[];
	const unsigned int cnt = h.hdr[Q], first = h.hdr[4 + Q];
	if (blockIdx.x * (unsigned int)BLOCK >= cnt) return;
	b = stage<KIND, true>(b, s_exp, s_pow, s_atan, s_rows, rows, n_mat, in_lds);
	const unsigned int stride = gridDim.x * (unsigned int)BLOCK;
	const unsigned int t = threadIdx.x;
	for (unsigned int j0 = blockIdx.x * (unsigned int)BLOCK; j0 < cnt; j0 += stride) {     // j0: workgroup-uniform
		const unsigned int j = j0 + t;
		const bool live = j < cnt;
		bool act = false;
		unsigned int id = 0u, k = 0u;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		if (live) {
			k = h.list[first + j];
			act = local_of(h, k, Q, n_mat, id);
			i = load3(vi, (long long)k); o = load3(vo, (long long)k);
			// above the horizon (the plugins' guard; a NaN z is evaluated): anything else reads neither row nor table
			act = act && !(i.z <= 0.0f || o.z <= 0.0f);
			if (!act) id = 0u;
		}
		v3 fr = mk(0, 0, 0); float pdf = 0.0f;                                     // below the horizon: +0
		if (__ballot(act) != 0ull) {                                               // wave-uniform
			if (act) {
				const Brdf pb = proxy_of(b, px, n_mat, id);
				v3 unused;
				mf_eval_pdf<KIND_TABULAR, 4>(pb, pp, i, o, unused, pdf);
				if (in_lds) unit<KIND, 2>(b, s_rows + id * STRIDE, i, o, fr);
				else unit<KIND, 2>(b, (const double *)((const char *)rows + (size_t)(id * (STRIDE * 8u))), i, o, fr);
			}
		}
		if (live) { out_pdf[k] = pdf; store3(vout, (long long)k, fr); }
	}
}

// ---- launches
// the partition of a chunk; LIGHT: va = out_fr
template <bool LIGHT>
hipError_t partition(hipStream_t s, const unsigned int *slots, int n_slots, long long m, const int32_t *mat, const View &va, const View &vb, float *out_pdf,
                     const djbk::SceneScratch &sc)
{
	const unsigned int n_tiles = (unsigned int)djbk::scene_tiles(m);
	hipError_t e = djbk::launch_scene_count_scan(s, slots, n_slots, m, mat, sc);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL((k_scene_scatter_proxy<LIGHT>), dim3((n_tiles + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, s, slots, (unsigned int)n_slots,
	                   (unsigned int)m, mat, n_tiles, sc.tiles, sc.list, va, vb, out_pdf);
	return hipGetLastError();
}

template <int PKIND>
hipError_t launch_lobe_is(hipStream_t s, const Hits &h, const djbk::SceneMembers &mb, const djbk::SceneProxies &px, const Brdf &pb, const dim3 &g,
                          const float *u1, const float *u2, const View &o, const View &out_w, const View &out_i, float *out_pdf, bool merl_exact)
{
	hipError_t e;
	if (mb.merl) {
		hipLaunchKernelGGL((k_scene_merl_is<PKIND>), g, dim3(BLOCK), 0, s, h, pb, px.merl, mb.merl, (unsigned int)mb.n_merl, u1, u2, o, out_w, out_i, out_pdf,
		                   MERL_GUARD_DEFAULT, merl_exact ? 1 : 0);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (mb.utia) {
		hipLaunchKernelGGL((k_scene_utia_is<PKIND>), g, dim3(BLOCK), 0, s, h, pb, utia_target(), px.utia, mb.utia, (unsigned int)mb.n_utia, u1, u2, o, out_w,
		                   out_i, out_pdf);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}
template <int PKIND>
hipError_t launch_lobe_light(hipStream_t s, const Hits &h, const djbk::SceneMembers &mb, const djbk::SceneProxies &px, const Brdf &pb, const dim3 &g,
                             const View &i, const View &o, const View &out, float *out_pdf, bool merl_exact)
{
	hipError_t e;
	if (mb.merl) {
		hipLaunchKernelGGL((k_scene_merl_light<PKIND>), g, dim3(BLOCK), 0, s, h, pb, px.merl, mb.merl, (unsigned int)mb.n_merl, i, o, out, out_pdf,
		                   MERL_GUARD_DEFAULT, merl_exact ? 1 : 0);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (mb.utia) {
		hipLaunchKernelGGL((k_scene_utia_light<PKIND>), g, dim3(BLOCK), 0, s, h, pb, utia_target(), px.utia, mb.utia, (unsigned int)mb.n_utia, i, o, out, out_pdf);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

template <int KIND>
hipError_t launch_model_is(hipStream_t s, const Hits &h, const double *rows, int n_mat, const ModelSetProxy &px, const Params &pp, bool rows_global,
                           const dim3 &g, const float *u1, const float *u2, const View &o, const View &out_w, const View &out_i, float *out_pdf)
{
	const ModelLaunch L(KIND, n_mat, rows_global, true);
	hipLaunchKernelGGL((k_scene_model_is<KIND>), g, dim3(BLOCK), L.lds, s, h, L.b, pp, px, rows, (unsigned int)n_mat, L.in_lds, u1, u2, o, out_w, out_i, out_pdf);
	return hipGetLastError();
}
template <int KIND>
hipError_t launch_model_light(hipStream_t s, const Hits &h, const double *rows, int n_mat, const ModelSetProxy &px, const Params &pp, bool rows_global,
                              const dim3 &g, const View &i, const View &o, const View &out, float *out_pdf)
{
	const ModelLaunch L(KIND, n_mat, rows_global, true);
	hipLaunchKernelGGL((k_scene_model_light<KIND>), g, dim3(BLOCK), L.lds, s, h, L.b, pp, px, rows, (unsigned int)n_mat, L.in_lds, i, o, out, out_pdf);
	return hipGetLastError();
}

// the lobe of the merl and utia parts: given and ggx or beckmann whenever the scene has such a member (the host's check)
bool lobe_ok(const djbk::SceneMembers &mb, const Brdf *proxy)
{
	if (!mb.merl && !mb.utia) return true;
	return proxy && (proxy->kind == KIND_GGX || proxy->kind == KIND_BECKMANN);
}

} // namespace

namespace djbk {

hipError_t launch_scene_evalp_is_proxy(hipStream_t s, const SceneMembers &mb, const SceneProxies &px, const Brdf *proxy, const Params &model_p,
                                       const unsigned int *slots, int n_slots, long long m, const int32_t *material, const float *u1, const float *u2,
                                       const View &o, const View &out_w, const View &out_i, float *out_pdf, const SceneScratch &sc, bool merl_exact,
                                       bool rows_global)
{
	if (m <= 0) return hipSuccess;
	if (m > SCENE_CHUNK_MAX || !lobe_ok(mb, proxy)) return hipErrorInvalidValue;
	hipError_t e = partition<false>(s, slots, n_slots, m, material, out_w, out_i, out_pdf, sc);
	if (e != hipSuccess) return e;
	const Hits h = { slots, (unsigned int)n_slots, material, sc.hdr, sc.list };
	const dim3 g(grid_capped(m, BLOCK, GRID_CAP));
	if (mb.merl || mb.utia) {
		e = proxy->kind == KIND_GGX ? launch_lobe_is<KIND_GGX>(s, h, mb, px, *proxy, g, u1, u2, o, out_w, out_i, out_pdf, merl_exact)
		                            : launch_lobe_is<KIND_BECKMANN>(s, h, mb, px, *proxy, g, u1, u2, o, out_w, out_i, out_pdf, merl_exact);
		if (e != hipSuccess) return e;
	}
	if (mb.sgd && (e = launch_model_is<KIND_SGD>(s, h, mb.sgd, mb.n_sgd, px.sgd, model_p, rows_global, g, u1, u2, o, out_w, out_i, out_pdf)) != hipSuccess) return e;
	if (mb.abc && (e = launch_model_is<KIND_ABC>(s, h, mb.abc, mb.n_abc, px.abc, model_p, rows_global, g, u1, u2, o, out_w, out_i, out_pdf)) != hipSuccess) return e;
	return hipSuccess;
}

hipError_t launch_scene_evalp_pdf_proxy(hipStream_t s, const SceneMembers &mb, const SceneProxies &px, const Brdf *proxy, const Params &model_p,
                                        const unsigned int *slots, int n_slots, long long m, const int32_t *material, const View &i, const View &o,
                                        const View &out_fr, float *out_pdf, const SceneScratch &sc, bool merl_exact, bool rows_global)
{
	if (m <= 0) return hipSuccess;
	if (m > SCENE_CHUNK_MAX || !lobe_ok(mb, proxy)) return hipErrorInvalidValue;
	hipError_t e = partition<true>(s, slots, n_slots, m, material, out_fr, out_fr, out_pdf, sc);
	if (e != hipSuccess) return e;
	const Hits h = { slots, (unsigned int)n_slots, material, sc.hdr, sc.list };
	const dim3 g(grid_capped(m, BLOCK, GRID_CAP));
	if (mb.merl || mb.utia) {
		e = proxy->kind == KIND_GGX ? launch_lobe_light<KIND_GGX>(s, h, mb, px, *proxy, g, i, o, out_fr, out_pdf, merl_exact)
		                            : launch_lobe_light<KIND_BECKMANN>(s, h, mb, px, *proxy, g, i, o, out_fr, out_pdf, merl_exact);
		if (e != hipSuccess) return e;
	}
	if (mb.sgd && (e = launch_model_light<KIND_SGD>(s, h, mb.sgd, mb.n_sgd, px.sgd, model_p, rows_global, g, i, o, out_fr, out_pdf)) != hipSuccess) return e;
	if (mb.abc && (e = launch_model_light<KIND_ABC>(s, h, mb.abc, mb.n_abc, px.abc, model_p, rows_global, g, i, o, out_fr, out_pdf)) != hipSuccess) return e;
	return hipSuccess;
}

} // namespace djbk
