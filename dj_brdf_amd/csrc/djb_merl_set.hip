// djb_merl_set.hip -- the C ABI of MERL material sets (include/djb_hip.h: djb_merl_set): M resident MERL tables in one block and one
// resolved proxy parameter set per material, evaluated / importance-sampled per hit by material id.  Kernels: djb_kernels_merl_set.hip;
// host loops (CPU contexts): djb_cpu.cpp; what the three kinds of set share: djb_set_host.hpp.  A set has no host twin: on a GPU context a
// host batch of any size is staged to the device.
#include "djb_set_host.hpp"

using namespace djbh;
using djbdev::MerlTexel;

namespace {

constexpr size_t TABLE_BYTES = sizeof(MerlTexel) * (size_t)MERL_N;

// the proxy of a proxy call (`op`, as the messages name it) is a ggx or beckmann object of the set's context, and the set has parameters for it
djb_status proxy_check(const djb_ctx *ctx, const djb_merl_set *s, const djb_brdf *proxy, const char *op)
{
	djb_status st = proxy_object_check(ctx, proxy, "merl set", op);
	if (st != DJB_OK) return st;
	if (!s->has_params) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the merl set has no proxy parameters (djb_merl_set_set_proxy_params)");
	return DJB_OK;
}

} // namespace

extern "C" {

djb_status djb_merl_set_create(djb_ctx *ctx, int n_materials, const djb_brdf *const *merls, const djb_params *proxy_params, djb_merl_set **out)
try {
	if (!ctx || !out || !merls) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	djb_status st = set_count_check("merl", n_materials, DJB_MERL_SET_MAX);
	if (st != DJB_OK) return st;
	const bool cpu = is_cpu(ctx);
	std::vector<const void *> src((size_t)n_materials);
	for (int m = 0; m < n_materials; ++m) {
		const djb_brdf *b = merls[m];
		if (cpu) { if ((st = djbcpu::merl_set_member(ctx, b, m, &src[m])) != DJB_OK) return st; continue; }
		if ((st = set_gpu_member(ctx, b, m, "merl")) != DJB_OK) return st;
		if (b->dev.kind != DJB_KIND_MERL || b->dev.merl_sparse || !b->dev.merl)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: merl set member %d is not a dense merl brdf (kind %d)", m, b->dev.kind);
		src[m] = b->dev.merl;
	}
	std::vector<Params> resolved;
	if (proxy_params && (st = resolve_all(cpu, n_materials, proxy_params, &resolved, "merl")) != DJB_OK) return st;

	djb_merl_set *s = set_new<djb_merl_set>(ctx, n_materials);
	const size_t tex_bytes = TABLE_BYTES * (size_t)n_materials, par_bytes = sizeof(Params) * (size_t)n_materials;
	if (cpu) {
		s->tex = (MerlTexel *)malloc(tex_bytes);
		s->params = (Params *)calloc((size_t)n_materials, sizeof(Params));
		if (!s->tex || !s->params) { djb_merl_set_destroy(s); return fail(DJB_ERR_OUT_OF_MEMORY, "djb_error: out of host memory (merl set of %d tables)", n_materials); }
		for (int m = 0; m < n_materials; ++m) memcpy(s->tex + (size_t)m * (size_t)MERL_N, src[m], TABLE_BYTES);
	} else if ((st = set_gpu_fill(s, djb_merl_set_destroy, "merl", n_materials, "tables", tex_bytes, [&] {
		hipError_t e = hipMalloc((void **)&s->params, par_bytes);
		if (e == hipSuccess) e = hipMemsetAsync(s->params, 0, par_bytes, ctx->stream);       // finished with the gather's synchronise
		return e == hipSuccess ? set_gather(ctx, (void **)&s->tex, TABLE_BYTES, src) : e;
	})) != DJB_OK) return st;
	if (proxy_params && (st = install_params(s, resolved)) != DJB_OK) { djb_merl_set_destroy(s); return st; }
	*out = s;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_merl_set_set_proxy_params(djb_merl_set *s, const djb_params *proxy_params)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null merl set");
	std::vector<Params> resolved;
	djb_status st = resolve_all(s->device < 0, s->n_mat, proxy_params, &resolved, "merl");
	if (st != DJB_OK) return st;
	return install_params(s, resolved);
}
DJB_ABI_CATCH

djb_status djb_merl_set_info(const djb_merl_set *s, int *n_materials, int *has_proxy_params)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null merl set");
	if (n_materials) *n_materials = s->n_mat;
	if (has_proxy_params) *has_proxy_params = s->has_params ? 1 : 0;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_merl_set_destroy(djb_merl_set *s)
try {
	return s ? set_free(s, s->tex, s->params) : DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_merl_set_eval_batch(djb_ctx *ctx, const djb_merl_set *s, int64_t n, const int32_t *material, const djb_vec3_view *i,
                                   const djb_vec3_view *o, int want_cos, const djb_vec3_view *out_fr, int mem)
try {
	djb_status st = set_check(ctx, s, "merl");
	if (st != DJB_OK) return st;
	if (is_cpu(ctx)) return djbcpu::merl_set_eval(ctx, s->tex, s->n_mat, n, material, i, o, want_cos, out_fr);
	SetBatch c(ctx, nullptr, n, mem, material, i, o, out_fr);
	if (c.st != DJB_OK) return c.st;
	HIP_TRY(djbk::launch_merl_set_eval(ctx->stream, s->tex, s->n_mat, n, c.dmat, c.vi, c.vo, c.vout, want_cos != 0, ctx->merl_exact_only != 0));
	return c.sg.finish();
}
DJB_ABI_CATCH

djb_status djb_merl_set_evalp_is_proxy_batch(djb_ctx *ctx, const djb_merl_set *s, const djb_brdf *proxy, int64_t n, const int32_t *material,
                                             const float *u1, const float *u2, const djb_vec3_view *o, const djb_vec3_view *out_weight,
                                             const djb_vec3_view *out_i, float *out_pdf, int mem)
try {
	djb_status st = set_check(ctx, s, "merl");
	if (st != DJB_OK) return st;
	if ((st = proxy_check(ctx, s, proxy, "evalp_is_proxy")) != DJB_OK) return st;
	if (is_cpu(ctx)) return djbcpu::merl_set_evalp_is_proxy(ctx, s->tex, s->params, s->n_mat, proxy, n, material, u1, u2, o, out_weight, out_i, out_pdf);
	SampleBatch c(ctx, proxy, n, mem, material, u1, u2, o, out_i, out_weight, out_pdf);
	if (c.st != DJB_OK) return c.st;
	HIP_TRY(djbk::launch_merl_set_evalp_is_proxy(ctx->stream, proxy->dev, s->params, s->tex, s->n_mat, n, c.dmat, c.d1, c.d2, c.vo, c.vw, c.vi, c.dpdf,
	                                             ctx->merl_exact_only != 0));
	return c.sg.finish();
}
DJB_ABI_CATCH

djb_status djb_merl_set_evalp_pdf_proxy_batch(djb_ctx *ctx, const djb_merl_set *s, const djb_brdf *proxy, int64_t n, const int32_t *material,
                                              const djb_vec3_view *i, const djb_vec3_view *o, const djb_vec3_view *out_fr, float *out_pdf, int mem)
try {
	djb_status st = set_check(ctx, s, "merl");
	if (st != DJB_OK) return st;
	if ((st = proxy_check(ctx, s, proxy, "evalp_pdf_proxy")) != DJB_OK) return st;
	if (!out_pdf) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null out_pdf (evalp alone: djb_merl_set_eval_batch)");
	if (is_cpu(ctx)) return djbcpu::merl_set_evalp_pdf(ctx, s->tex, s->params, s->n_mat, proxy, n, material, i, o, out_fr, out_pdf);
	SetBatch c(ctx, proxy, n, mem, material, i, o, out_fr);
	if (c.st != DJB_OK) return c.st;
	float *dpdf = nullptr;
	if ((st = c.sg.out_arr(out_pdf, &dpdf)) != DJB_OK) return st;
	HIP_TRY(djbk::launch_merl_set_evalp_pdf(ctx->stream, proxy->dev, s->params, s->tex, s->n_mat, n, c.dmat, c.vi, c.vo, c.vout, dpdf,
	                                        ctx->merl_exact_only != 0));
	return c.sg.finish();
}
DJB_ABI_CATCH

} // extern "C"
