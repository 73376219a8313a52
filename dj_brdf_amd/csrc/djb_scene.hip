// djb_scene.hip -- the C ABI of scenes (include/djb_hip.h: djb_scene): a resident slot table that maps a scene material id to (kind, local
// id) in up to four member sets -- a MERL set, a UTIA set, an sgd and an abc model set -- evaluated per hit in one call.  The scene borrows
// its members and copies only the slot table.  Kernels: djb_kernels_scene.hip (eval / evalp), djb_kernels_scene_proxy.hip (the sampling step
// and the light sample); host loops (CPU contexts): djb_cpu.cpp; the checks and the entry of a batch: djb_set_host.hpp.  A scene has no host
// twin: on a GPU context a host batch of any size is staged to the device.
#include "djb_set_host.hpp"

using namespace djbh;

namespace {

constexpr long long SCENE_CHUNK = 1LL << 24;     // hits per chunk: 64 MB of index list; indices and list positions stay far below 2^31
static_assert(SCENE_CHUNK <= djbk::SCENE_CHUNK_MAX && DJB_SCENE_MAX_SLOTS <= (1 << 30), "chunk and table sizes the kernels' 32-bit indices hold");

// kind of the ABI -> the kernels' code (djb_internal.hpp), or -1
int kind_code(int kind)
{
	switch (kind) {
	case DJB_KIND_MERL: return 0;
	case DJB_KIND_UTIA: return 1;
	case DJB_KIND_SGD: return 2;
	case DJB_KIND_ABC: return 3;
	}
	return -1;
}

djbk::SceneMembers members_of(const djb_scene *s)
{
	return { s->merl ? s->merl->tex : nullptr, s->merl ? s->merl->n_mat : 0, s->utia ? s->utia->tab : nullptr, s->utia ? s->utia->n_mat : 0,
	         s->sgd ? s->sgd->rows : nullptr, s->sgd ? s->sgd->n_mat : 0, s->abc ? s->abc->rows : nullptr, s->abc ? s->abc->n_mat : 0 };
}

// The partition's list, the tile counts, count / offset and the utia worklist share the context's scratch, sized once for the largest
// chunk of a call of n hits: words [0, 8) count[4] offset[4], [8, 12) the worklist's count, from 16: tiles, list, worklist (wl_cap entries;
// the proxy calls have none).  *chunk: the hits per chunk
djb_status scene_scratch(djb_ctx *ctx, long long n, size_t wl_cap, long long *chunk, djbk::SceneScratch *sc)
{
	*chunk = ctx->test_scene_chunk > 0 ? ctx->test_scene_chunk : SCENE_CHUNK;                      // DJB_OPT_TEST_SCENE_CHUNK (tests)
	const long long mc = std::min<long long>(n, *chunk);
	const size_t tiles = 4 * djbk::scene_tiles(mc);
	djb_status st = ensure_scratch(ctx, 4 * (16 + tiles + (size_t)mc + (wl_cap ? wl_cap : 1)));
	if (st != DJB_OK) return st;
	unsigned int *w = (unsigned int *)ctx->scratch;
	*sc = { w, w + 16, w + 16 + tiles, w + 8, w + 16 + tiles + (size_t)mc, (unsigned int)wl_cap };
	return DJB_OK;
}
// a call of n hits: launch(lo, m, sc) for the m hits from `lo` on, chunk after chunk, back to back on the context's stream
template <class Launch> djb_status scene_chunks(djb_ctx *ctx, long long n, size_t wl_cap, Launch launch)
{
	if (n <= 0) return DJB_OK;
	long long chunk;
	djbk::SceneScratch sc;
	djb_status st = scene_scratch(ctx, n, wl_cap, &chunk, &sc);
	if (st != DJB_OK) return st;
	for (long long lo = 0; lo < n; lo += chunk) HIP_TRY(launch(lo, std::min(n - lo, chunk), sc));
	return DJB_OK;
}

// What the two proxy calls ask of the scene's MEMBERS, before anything is launched: a ggx or beckmann `proxy` of the call's context when
// there is a merl or utia member (the text of the MERL set's proxy_check), and on every member the block its hits will read
djb_status proxy_members_check(const djb_ctx *ctx, const djb_scene *s, const djb_brdf *proxy, const char *op)
{
	djb_status st;
	if ((s->merl || s->utia) && (st = proxy_object_check(ctx, proxy, "scene", op)) != DJB_OK) return st;
	if (s->merl && !s->merl->has_params)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the scene's merl member has no proxy parameters (djb_merl_set_set_proxy_params)");
	if (s->utia && !s->utia->has_params)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the scene's utia member has no proxy parameters (djb_utia_set_set_proxy_params)");
	if (s->sgd && !s->sgd->proxy_res) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the scene's sgd member has no proxy (djb_model_set_fit_proxy)");
	if (s->abc && !s->abc->proxy_res) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the scene's abc member has no proxy (djb_model_set_fit_proxy)");
	return DJB_OK;
}
// the members' CURRENT parameter blocks and proxy tables: read at every call, the scene keeps no copy
djbk::SceneProxies proxies_of(const djb_scene *s)
{
	djbk::SceneProxies p = { s->merl ? s->merl->params : nullptr, s->utia ? s->utia->params : nullptr, { nullptr, 0, 0 }, { nullptr, 0, 0 } };
	if (s->sgd) p.sgd = { s->sgd->proxy_dev, s->sgd->proxy_res, s->sgd->proxy_shadow };
	if (s->abc) p.abc = { s->abc->proxy_dev, s->abc->proxy_res, s->abc->proxy_shadow };
	return p;
}
djbcpu::SceneHost host_of(const djb_scene *s)
{
	djbcpu::SceneHost h = {};
	h.slots = s->slots; h.n_slots = s->n_mat;
	if (s->merl) { h.merl_texels = s->merl->tex; h.merl_params = s->merl->params; }
	if (s->utia) { h.utia_records = s->utia->tab; h.utia_params = s->utia->params; }
	if (s->sgd) { h.sgd_rows = s->sgd->rows; h.sgd_block = s->sgd->proxy_host.data(); h.n_sgd = s->sgd->n_mat; h.sgd_res = s->sgd->proxy_res; h.sgd_shadow = s->sgd->proxy_shadow; }
	if (s->abc) { h.abc_rows = s->abc->rows; h.abc_block = s->abc->proxy_host.data(); h.n_abc = s->abc->n_mat; h.abc_res = s->abc->proxy_res; h.abc_shadow = s->abc->proxy_shadow; }
	return h;
}

} // namespace

extern "C" {

djb_status djb_scene_create(djb_ctx *ctx, const djb_merl_set *merl, const djb_utia_set *utia, const djb_model_set *sgd, const djb_model_set *abc,
                            int n_slots, const djb_scene_slot *slots, djb_scene **out)
try {
	if (!ctx || !out || !slots) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	if (!merl && !utia && !sgd && !abc) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a scene needs at least one member set");
	if (n_slots < 1 || n_slots > DJB_SCENE_MAX_SLOTS)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a scene holds 1 .. %d slots (got %d)", DJB_SCENE_MAX_SLOTS, n_slots);
	djb_status st;
	if (merl && (st = set_check(ctx, merl, "merl")) != DJB_OK) return st;
	if (utia && (st = set_check(ctx, utia, "utia")) != DJB_OK) return st;
	if (sgd && (st = set_check(ctx, sgd, "model")) != DJB_OK) return st;
	if (abc && (st = set_check(ctx, abc, "model")) != DJB_OK) return st;
	if (sgd && sgd->kind != DJB_KIND_SGD) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the scene's sgd member is a model set of kind %d", sgd->kind);
	if (abc && abc->kind != DJB_KIND_ABC) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the scene's abc member is a model set of kind %d", abc->kind);
	const int count[4] = { merl ? merl->n_mat : 0, utia ? utia->n_mat : 0, sgd ? sgd->n_mat : 0, abc ? abc->n_mat : 0 };
	static const char *const name[4] = { "merl", "utia", "sgd", "abc" };
	std::vector<unsigned int> words((size_t)n_slots);
	for (int k = 0; k < n_slots; ++k) {
		if (slots[k].kind == DJB_SCENE_NONE) { words[k] = 0xffffffffu; continue; }
		const int q = kind_code(slots[k].kind);
		if (q < 0) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: scene slot %d names kind %d (merl, utia, sgd, abc or DJB_SCENE_NONE)", k, slots[k].kind);
		if (!count[q]) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: scene slot %d names a %s material, but the scene has no %s set", k, name[q], name[q]);
		if (slots[k].local < 0 || slots[k].local >= count[q] || slots[k].local > 65535)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: scene slot %d names %s material %d, outside the set's 0 .. %d", k, name[q], slots[k].local,
			            std::min(count[q], 65536) - 1);
		words[k] = ((unsigned int)q << 16) | (unsigned int)slots[k].local;
	}
	djb_scene *s = set_new<djb_scene>(ctx, n_slots);
	s->merl = merl; s->utia = utia; s->sgd = sgd; s->abc = abc;
	const size_t bytes = sizeof(unsigned int) * words.size();
	if (is_cpu(ctx)) {
		s->slots = (unsigned int *)malloc(bytes);
		if (!s->slots) { djb_scene_destroy(s); return fail(DJB_ERR_OUT_OF_MEMORY, "djb_error: out of host memory (scene of %d slots)", n_slots); }
		memcpy(s->slots, words.data(), bytes);
	} else if ((st = set_gpu_fill(s, djb_scene_destroy, "scene", n_slots, "slots", bytes, [&] {
		hipError_t e = hipMalloc((void **)&s->slots, bytes);
		return e == hipSuccess ? hipMemcpy(s->slots, words.data(), bytes, hipMemcpyHostToDevice) : e;     // synchronous: `words` goes out of scope
	})) != DJB_OK) return st;
	*out = s;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_scene_info(const djb_scene *s, int *n_slots, int members[4])
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null scene");
	if (n_slots) *n_slots = s->n_mat;
	if (members) {
		members[0] = s->merl ? s->merl->n_mat : 0; members[1] = s->utia ? s->utia->n_mat : 0;
		members[2] = s->sgd ? s->sgd->n_mat : 0; members[3] = s->abc ? s->abc->n_mat : 0;
	}
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_scene_destroy(djb_scene *s)
try {
	return s ? set_free(s, s->slots) : DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_scene_eval_batch(djb_ctx *ctx, const djb_scene *s, int64_t n, const int32_t *material, const djb_vec3_view *i, const djb_vec3_view *o,
                                int want_cos, const djb_vec3_view *out_fr, int mem)
try {
	djb_status st = set_check(ctx, s, "scene");
	if (st != DJB_OK) return st;
	if (is_cpu(ctx))
		return djbcpu::scene_eval(ctx, host_of(s), n, material, i, o, want_cos, out_fr);
	SetBatch c(ctx, nullptr, n, mem, material, i, o, out_fr);
	if (c.st != DJB_OK) return c.st;
	const View &vi = c.vi, &vo = c.vo, &vout = c.vout;
	// Every lane reads its hit before it writes it and kinds touch disjoint hits, so index-aligned in-place views are supported.  The utia
	// fix pass reads a hit again after tier 1 stored it: a device-resident caller whose outputs overlap an input stream, the ids included,
	// gets the exact kernel alone for the utia part (the rule of djb_utia_set_eval_batch)
	const Stream ins[7] = { { vi.x, vi.stride }, { vi.y, vi.stride }, { vi.z, vi.stride }, { vo.x, vo.stride }, { vo.y, vo.stride }, { vo.z, vo.stride },
	                        { c.dmat, 1 } };
	const Stream outs[3] = { { vout.x, vout.stride }, { vout.y, vout.stride }, { vout.z, vout.stride } };
	const bool utia_exact = ctx->utia_exact_only != 0 || (mem == DJB_MEM_DEVICE && outputs_overlap_inputs(n, ins, 7, outs, 3));
	const djbk::SceneMembers mb = members_of(s);
	size_t cap = (size_t)(std::min<long long>(n, ctx->test_scene_chunk > 0 ? ctx->test_scene_chunk : SCENE_CHUNK) / 256 + 4096);
	if (ctx->test_worklist_cap >= 0) cap = (size_t)ctx->test_worklist_cap;                         // DJB_OPT_TEST_WORKLIST_CAP (tests): force the overflow path
	if ((st = scene_chunks(ctx, n, cap, [&](long long lo, long long m, const djbk::SceneScratch &sc) {
		return djbk::launch_scene_eval(ctx->stream, mb, s->slots, s->n_mat, m, c.dmat + lo, offset_view(vi, lo), offset_view(vo, lo), offset_view(vout, lo),
		                               want_cos != 0, sc, ctx->merl_exact_only != 0, utia_exact, ctx->model_set_rows_global != 0);
	})) != DJB_OK) return st;
	return c.sg.finish();
}
DJB_ABI_CATCH

// Overlap: index-aligned in-place views only.  Every lane reads its hit before it writes it, kinds touch disjoint hits, the MERL drains work
// on their queued records and no kernel here takes a second pass over a hit, so nothing needs the exact-only detour of the eval call
djb_status djb_scene_evalp_is_proxy_batch(djb_ctx *ctx, const djb_scene *s, const djb_brdf *proxy, int64_t n, const int32_t *material, const float *u1,
                                          const float *u2, const djb_vec3_view *o, const djb_vec3_view *out_weight, const djb_vec3_view *out_i,
                                          float *out_pdf, int mem)
try {
	djb_status st = set_check(ctx, s, "scene");
	if (st != DJB_OK) return st;
	if ((st = proxy_members_check(ctx, s, proxy, "evalp_is_proxy")) != DJB_OK) return st;
	const djb_brdf *lobe = s->merl || s->utia ? proxy : nullptr;                                   // not looked at without such a member
	if (is_cpu(ctx)) return djbcpu::scene_evalp_is_proxy(ctx, host_of(s), lobe, n, material, u1, u2, o, out_weight, out_i, out_pdf);
	if (!Staged::valid(out_weight) || !Staged::valid(out_i) || !out_pdf) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null output");
	Params model_p;
	if ((st = device_params(nullptr, &model_p, DJB_KIND_TABULAR)) != DJB_OK) return st;            // as the model set's call resolves it
	SampleBatch c(ctx, lobe, n, mem, material, u1, u2, o, out_i, out_weight, out_pdf);
	if (c.st != DJB_OK) return c.st;
	const djbk::SceneMembers mb = members_of(s);
	const djbk::SceneProxies px = proxies_of(s);
	if ((st = scene_chunks(ctx, n, 0, [&](long long lo, long long m, const djbk::SceneScratch &sc) {
		return djbk::launch_scene_evalp_is_proxy(ctx->stream, mb, px, lobe ? &lobe->dev : nullptr, model_p, s->slots, s->n_mat, m, c.dmat + lo, c.d1 + lo,
		                                         c.d2 + lo, offset_view(c.vo, lo), offset_view(c.vw, lo), offset_view(c.vi, lo), c.dpdf + lo, sc,
		                                         ctx->merl_exact_only != 0, ctx->model_set_rows_global != 0);
	})) != DJB_OK) return st;
	return c.sg.finish();
}
DJB_ABI_CATCH

djb_status djb_scene_evalp_pdf_proxy_batch(djb_ctx *ctx, const djb_scene *s, const djb_brdf *proxy, int64_t n, const int32_t *material,
                                           const djb_vec3_view *i, const djb_vec3_view *o, const djb_vec3_view *out_fr, float *out_pdf, int mem)
try {
	djb_status st = set_check(ctx, s, "scene");
	if (st != DJB_OK) return st;
	if ((st = proxy_members_check(ctx, s, proxy, "evalp_pdf_proxy")) != DJB_OK) return st;
	if (!out_pdf) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null out_pdf (evalp alone: djb_scene_eval_batch)");
	const djb_brdf *lobe = s->merl || s->utia ? proxy : nullptr;                                   // not looked at without such a member
	if (is_cpu(ctx)) return djbcpu::scene_evalp_pdf(ctx, host_of(s), lobe, n, material, i, o, out_fr, out_pdf);
	Params model_p;
	if ((st = device_params(nullptr, &model_p, DJB_KIND_TABULAR)) != DJB_OK) return st;
	SetBatch c(ctx, lobe, n, mem, material, i, o, out_fr);
	if (c.st != DJB_OK) return c.st;
	float *dpdf = nullptr;
	if ((st = c.sg.out_arr(out_pdf, &dpdf)) != DJB_OK) return st;
	const djbk::SceneMembers mb = members_of(s);
	const djbk::SceneProxies px = proxies_of(s);
	if ((st = scene_chunks(ctx, n, 0, [&](long long lo, long long m, const djbk::SceneScratch &sc) {
		return djbk::launch_scene_evalp_pdf_proxy(ctx->stream, mb, px, lobe ? &lobe->dev : nullptr, model_p, s->slots, s->n_mat, m, c.dmat + lo,
		                                          offset_view(c.vi, lo), offset_view(c.vo, lo), offset_view(c.vout, lo), dpdf + lo, sc,
		                                          ctx->merl_exact_only != 0, ctx->model_set_rows_global != 0);
	})) != DJB_OK) return st;
	return c.sg.finish();
}
DJB_ABI_CATCH

} // extern "C"
