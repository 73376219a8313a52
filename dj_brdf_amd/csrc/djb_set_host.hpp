// djb_set_host.hpp -- what the C ABIs of the four material sets and of scenes share (djb_merl_set.hip, djb_utia_set.hip, djb_model_set.hip,
// djb_microfacet_set.hip, djb_scene.hip; included by those alone): the checks of a handle, a member and a count, the construction and release of the resident block,
// the proxy parameter block of the MERL and UTIA sets and the check of a proxy object, and the entry of a batch of either shape (eval or
// light sample; sampling).  `what` is the set's noun in the messages: "merl" / "utia" / "model" / "microfacet" / "scene".  Everything works on
// djb_set_base (djb_host.hpp).
#pragma once
#include "djb_host.hpp"

namespace djbh {

// the set belongs to the call's context, as a djb_brdf does
inline djb_status set_check(const djb_ctx *ctx, const djb_set_base *s, const char *what)
{
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null %s set", what);
	if (!ctx) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null ctx");
	if (is_cpu(ctx) != (s->device < 0))
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: %s set and ctx belong to different back ends (CPU / GPU)", what);
	if (s->ctx != ctx) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the %s set belongs to another context", what);
	return DJB_OK;
}
inline djb_status set_count_check(const char *what, int n, int max)
{
	if (n < 1 || n > max) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a %s set holds 1 .. %d materials (got %d)", what, max, n);
	return DJB_OK;
}
// member m of a GPU context's set is an object of that context (a CPU context's: djbcpu::*_set_member); its kind is each set's own test
inline djb_status set_gpu_member(const djb_ctx *ctx, const djb_brdf *b, int m, const char *what)
{
	if (!b) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: %s set member %d is a null brdf", what, m);
	if (is_cpu(b) || b->ctx != ctx || b->device != ctx->device)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: %s set member %d belongs to another context", what, m);
	return DJB_OK;
}

template <class S> S *set_new(djb_ctx *ctx, int n_mat)
{
	S *s = new S();
	s->device = is_cpu(ctx) ? -1 : ctx->device;
	s->ctx = ctx;
	s->n_mat = n_mat;
	return s;
}
// the handle and its blocks, which live where the set's context computes
template <class S, class... P> djb_status set_free(S *s, P *... blocks)
{
	if (s->device < 0) (free(blocks), ...);
	else {
		(void)hipSetDevice(s->device);
		((blocks ? (void)hipFree(blocks) : (void)0), ...);
	}
	delete s;
	return DJB_OK;
}
// A GPU set's resident block: `fill` allocates and fills it under the context's call lock and returns when the data is in place.  On an
// error the set is destroyed; the message names `n` `unit`s ("tables" / "rows") and `bytes`.
template <class S, class Fill>
djb_status set_gpu_fill(S *s, djb_status (*destroy)(S *), const char *what, int n, const char *unit, size_t bytes, Fill fill)
{
	djb_ctx *ctx = s->ctx;
	djb_status st = check_call(ctx, nullptr, 0, DJB_MEM_DEVICE);
	if (st != DJB_OK) { delete s; return st; }
	std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
	const hipError_t e = fill();
	if (e == hipSuccess) return DJB_OK;
	(void)hipGetLastError();
	(void)hipStreamSynchronize(ctx->stream);
	destroy(s);
	return fail(DJB_ERR_HIP, "djb_error: HIP allocation / copy of a %s set of %d %s (%zu bytes): %s", what, n, unit, bytes, hipGetErrorString(e));
}
// a fill: one block on the context's device, the equally sized device-resident sources gathered into it one after the other on the
// context's stream; synchronised, so the sources may be destroyed as soon as this returns
inline hipError_t set_gather(djb_ctx *ctx, void **block, size_t each, const std::vector<const void *> &src)
{
	hipError_t e = hipMalloc(block, each * src.size());
	for (size_t m = 0; m < src.size() && e == hipSuccess; ++m)
		e = hipMemcpyAsync((char *)*block + m * each, src[m], each, hipMemcpyDeviceToDevice, ctx->stream);
	return e == hipSuccess ? hipStreamSynchronize(ctx->stream) : e;
}

// ---- the proxy parameter block of a MERL or UTIA set: n_mat plain parameter sets -> Params as the single-material calls of the set's back
// end resolve them (`what`: "merl" / "utia")
inline djb_status resolve_all(bool cpu, int n_mat, const djb_params *in, std::vector<Params> *out, const char *what)
{
	if (!in) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null proxy_params");
	out->resize((size_t)n_mat);
	for (int m = 0; m < n_mat; ++m) {
		if (in[m].kind & DJB_PARAMS_RESOLVED_FOLLOWS)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: proxy_params[%d] carries DJB_PARAMS_RESOLVED_FOLLOWS: a %s set takes plain djb_params", m, what);
		memset(&(*out)[m], 0, sizeof(Params));
		djb_status st = cpu ? djbcpu::merl_set_resolve_params(&in[m], &(*out)[m]) : device_params(&in[m], &(*out)[m], DJB_KIND_GGX);
		if (st != DJB_OK) return st;
	}
	return DJB_OK;
}
// replaces the resident parameters (s->params holds n_mat Params); a GPU set: one copy on the context's stream, finished when this returns
template <class S> djb_status install_params(S *s, const std::vector<Params> &p)
{
	if (s->device < 0) { memcpy(s->params, p.data(), sizeof(Params) * p.size()); s->has_params = true; return DJB_OK; }
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::recursive_mutex> call_lock(s->ctx->call_mu);
	HIP_TRY(hipMemcpyAsync(s->params, p.data(), sizeof(Params) * p.size(), hipMemcpyHostToDevice, s->ctx->stream));
	HIP_TRY(hipStreamSynchronize(s->ctx->stream));        // `p` is pageable host memory of the caller's frame
	s->has_params = true;
	return DJB_OK;
}
// the proxy of a per-hit proxy call (`op`, as the messages name it) on `what` ("merl set" / "scene"): a ggx or beckmann object of the call's context
inline djb_status proxy_object_check(const djb_ctx *ctx, const djb_brdf *proxy, const char *what, const char *op)
{
	if (!proxy) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null brdf (proxy)");
	djb_status st = cpu_pair_check(ctx, proxy);
	if (st != DJB_OK) return st;
	const bool cpu = is_cpu(ctx);
	if (!cpu && (proxy->ctx != ctx || proxy->device != ctx->device))
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: %s and proxy belong to different contexts", what);
	const int pkind = cpu ? djbcpu::kind(proxy) : proxy->dev.kind;
	if (pkind != DJB_KIND_GGX && pkind != DJB_KIND_BECKMANN)
		return fail(DJB_ERR_NOT_IMPLEMENTED, "djb_error: %s on a %s takes a ggx or beckmann proxy (proxy kind %d)", op, what, pkind);
	return DJB_OK;
}

// The entry of a batch call on a GPU context's set, after set_check and the CPU dispatch: check_call, the call lock (held while this
// object lives), then the call's arrays where the kernels read and write them, staged by the two shapes below.  `st` is the first
// failure; the caller launches on the staged members and returns sg.finish().
struct BatchEntry {
	djb_status st;
	std::unique_lock<std::recursive_mutex> call_lock;
	Staged sg;
	const int32_t *dmat = nullptr;

	BatchEntry(djb_ctx *ctx, const djb_brdf *b, long long n, int mem)
		: st(check_call(ctx, b, n, mem)),
		  call_lock(st == DJB_OK ? std::unique_lock<std::recursive_mutex>(ctx->call_mu) : std::unique_lock<std::recursive_mutex>()),
		  sg(ctx, n, mem) {}
};
// an eval or light-sample batch: the ids, i, o and the output (a light sample's out_pdf: the caller's, after this)
struct SetBatch : BatchEntry {
	View vi, vo, vout;

	SetBatch(djb_ctx *ctx, const djb_brdf *b, long long n, int mem, const int32_t *material, const djb_vec3_view *i, const djb_vec3_view *o,
	         const djb_vec3_view *out)
		: BatchEntry(ctx, b, n, mem)
	{
		if (st != DJB_OK) return;
		if ((st = stage_material(sg, material, &dmat)) != DJB_OK) return;
		if ((st = sg.in_vec(i, &vi)) != DJB_OK) return;
		if ((st = sg.in_vec(o, &vo)) != DJB_OK) return;
		st = sg.out_vec(out, &vout);
	}
};
// a sampling batch: the ids, u1, u2, o, then the outputs i, weight and pdf
struct SampleBatch : BatchEntry {
	const float *d1 = nullptr, *d2 = nullptr;
	View vo, vi, vw;
	float *dpdf = nullptr;

	SampleBatch(djb_ctx *ctx, const djb_brdf *b, long long n, int mem, const int32_t *material, const float *u1, const float *u2, const djb_vec3_view *o,
	            const djb_vec3_view *out_i, const djb_vec3_view *out_weight, float *out_pdf)
		: BatchEntry(ctx, b, n, mem)
	{
		if (st != DJB_OK) return;
		if ((st = stage_material(sg, material, &dmat)) != DJB_OK) return;
		if ((st = sg.in_f(u1, &d1)) != DJB_OK) return;
		if ((st = sg.in_f(u2, &d2)) != DJB_OK) return;
		if ((st = sg.in_vec(o, &vo)) != DJB_OK) return;
		if ((st = sg.out_vec(out_i, &vi)) != DJB_OK) return;
		if ((st = sg.out_vec(out_weight, &vw)) != DJB_OK) return;
		st = sg.out_arr(out_pdf, &dpdf);
	}
};

} // namespace djbh
