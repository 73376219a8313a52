// djb_microfacet_set.hip -- the C ABI of microfacet sets (include/djb_hip.h: djb_microfacet_set): M resident analytic materials of one NDF
// kind, ggx or beckmann -- resolved parameters, Fresnel term and shadowing flag each, one MfRow (djb_microfacet_row.hpp) -- evaluated and
// sampled per hit by material id.  Kernels: djb_kernels_microfacet_set.hip; host loops (CPU contexts): djb_cpu.cpp; what the sets share:
// djb_set_host.hpp.  A set has no host twin: on a GPU context a host batch of any size is staged to the device.
#include "djb_set_host.hpp"

using namespace djbh;
using djbdev::MfRow;

namespace {

const char *kind_name(int kind) { return kind == DJB_KIND_GGX ? "ggx" : kind == DJB_KIND_BECKMANN ? "beckmann" : "?"; }

// the Fresnel term of material m as a row keeps it
djb_status fresnel_check(const djb_fresnel_desc &f, int m)
{
	switch (f.kind) {
	case DJB_FRESNEL_IDEAL: case DJB_FRESNEL_UNPOLARIZED: case DJB_FRESNEL_SCHLICK: case DJB_FRESNEL_SGD: return DJB_OK;
	case DJB_FRESNEL_SPLINE:
		return fail(DJB_ERR_NOT_IMPLEMENTED, "djb_error: microfacet set material %d has a spline Fresnel term: a row holds ideal, unpolarized, schlick or sgd", m);
	case DJB_FRESNEL_HOST:
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: microfacet set material %d has a host-evaluated Fresnel term (DJB_FRESNEL_HOST)", m);
	default: return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: microfacet set material %d: unknown fresnel kind %d", m, f.kind);
	}
}

// the rows of n materials, the parameters resolved as the single-material call of the set's back end resolves them (resolve_all)
djb_status build_rows(bool cpu, int n, const djb_microfacet_material *mats, std::vector<MfRow> *rows, int *fr_kind)
{
	std::vector<djb_params> plain((size_t)n);
	for (int m = 0; m < n; ++m) {
		djb_status st = fresnel_check(mats[m].fresnel, m);
		if (st != DJB_OK) return st;
		plain[m] = mats[m].params;
	}
	std::vector<Params> p;
	djb_status st = resolve_all(cpu, n, plain.data(), &p, "microfacet");
	if (st != DJB_OK) return st;
	rows->resize((size_t)n);
	*fr_kind = mats[0].fresnel.kind;
	for (int m = 0; m < n; ++m) {
		MfRow &r = (*rows)[m];
		memset(&r, 0, sizeof r);                                                   // the padding too: the block is compared and copied as bytes
		r.p = p[m];
		r.fr_kind = mats[m].fresnel.kind;
		for (int c = 0; c < 3; ++c) { r.a[c] = mats[m].fresnel.a[c]; r.b[c] = mats[m].fresnel.b[c]; }
		r.shadow = mats[m].shadow != 0;
		if (r.fr_kind != *fr_kind) *fr_kind = -1;
	}
	return DJB_OK;
}

djb_status create(djb_ctx *ctx, int kind, int n, const djb_microfacet_material *mats, djb_microfacet_set **out)
{
	const bool cpu = is_cpu(ctx);
	std::vector<MfRow> rows;
	int fr_kind = -1;
	djb_status st = build_rows(cpu, n, mats, &rows, &fr_kind);
	if (st != DJB_OK) return st;
	djb_microfacet_set *s = set_new<djb_microfacet_set>(ctx, n);
	s->kind = kind; s->fr_kind = fr_kind;
	const size_t bytes = sizeof(MfRow) * rows.size();
	if (cpu) {
		s->rows = (MfRow *)malloc(bytes);
		if (!s->rows) { djb_microfacet_set_destroy(s); return fail(DJB_ERR_OUT_OF_MEMORY, "djb_error: out of host memory (microfacet set of %d rows)", n); }
		memcpy(s->rows, rows.data(), bytes);
	} else {
		st = set_gpu_fill(s, djb_microfacet_set_destroy, "microfacet", n, "rows", bytes, [&] {
			hipError_t e = hipMalloc((void **)&s->rows, bytes);
			return e == hipSuccess ? hipMemcpy(s->rows, rows.data(), bytes, hipMemcpyHostToDevice) : e;     // synchronous: `rows` is moved below
		});
		if (st != DJB_OK) return st;
		s->host_rows.swap(rows);                                                   // what set_params keeps of every row
	}
	*out = s;
	return DJB_OK;
}

} // namespace

extern "C" {

djb_status djb_microfacet_set_create(djb_ctx *ctx, int kind, int n_materials, const djb_microfacet_material *materials, djb_microfacet_set **out)
try {
	if (!ctx || !out || !materials) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	if (kind != DJB_KIND_GGX && kind != DJB_KIND_BECKMANN)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a microfacet set is of kind beckmann (%d) or ggx (%d) (got %d)", DJB_KIND_BECKMANN, DJB_KIND_GGX, kind);
	djb_status st = set_count_check("microfacet", n_materials, DJB_MICROFACET_SET_MAX);
	if (st != DJB_OK) return st;
	return create(ctx, kind, n_materials, materials, out);
}
DJB_ABI_CATCH

djb_status djb_microfacet_set_create_from_brdfs(djb_ctx *ctx, int n_materials, const djb_brdf *const *members, const djb_params *params,
                                                djb_microfacet_set **out)
try {
	if (!ctx || !out || !members) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	djb_status st = set_count_check("microfacet", n_materials, DJB_MICROFACET_SET_MAX);
	if (st != DJB_OK) return st;
	const bool cpu = is_cpu(ctx);
	int kind = -1;
	std::vector<djb_microfacet_material> mats((size_t)n_materials);
	for (int m = 0; m < n_materials; ++m) {
		const djb_brdf *b = members[m];
		djb_microfacet_material &mat = mats[m];
		memset(&mat, 0, sizeof mat);
		int k = -1;
		if (cpu) { if ((st = djbcpu::microfacet_set_member(ctx, b, m, &k, &mat.shadow, &mat.fresnel)) != DJB_OK) return st; }
		else {
			if ((st = set_gpu_member(ctx, b, m, "microfacet")) != DJB_OK) return st;
			k = b->dev.kind;
			mat.shadow = b->dev.shadow;
			mat.fresnel.kind = b->dev.fr.kind;
			for (int c = 0; c < 3; ++c) { mat.fresnel.a[c] = b->dev.fr.a[c]; mat.fresnel.b[c] = b->dev.fr.b[c]; }
		}
		if (k != DJB_KIND_GGX && k != DJB_KIND_BECKMANN)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: microfacet set member %d is not a ggx or beckmann brdf (kind %d)", m, k);
		if (m == 0) kind = k;
		else if (k != kind)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: microfacet set member %d is a %s brdf, member 0 a %s one (a set holds one kind)", m, kind_name(k),
			            kind_name(kind));
		if (params) mat.params = params[m];                                        // else zeroed: DJB_PARAMS_STANDARD
	}
	return create(ctx, kind, n_materials, mats.data(), out);
}
DJB_ABI_CATCH

djb_status djb_microfacet_set_set_params(djb_microfacet_set *s, const djb_params *params)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null microfacet set");
	if (!params) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null params");
	const bool cpu = s->device < 0;
	std::vector<Params> p;
	djb_status st = resolve_all(cpu, s->n_mat, params, &p, "microfacet");
	if (st != DJB_OK) return st;
	if (cpu) { for (int m = 0; m < s->n_mat; ++m) s->rows[m].p = p[(size_t)m]; return DJB_OK; }
	// one copy of the block on the context's stream, finished when this returns: stream order, as djb_merl_set_set_proxy_params
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::recursive_mutex> call_lock(s->ctx->call_mu);
	for (int m = 0; m < s->n_mat; ++m) s->host_rows[(size_t)m].p = p[(size_t)m];
	HIP_TRY(hipMemcpyAsync(s->rows, s->host_rows.data(), sizeof(MfRow) * s->host_rows.size(), hipMemcpyHostToDevice, s->ctx->stream));
	HIP_TRY(hipStreamSynchronize(s->ctx->stream));
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_microfacet_set_info(const djb_microfacet_set *s, int *kind, int *n_materials)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null microfacet set");
	if (kind) *kind = s->kind;
	if (n_materials) *n_materials = s->n_mat;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_microfacet_set_destroy(djb_microfacet_set *s)
try {
	return s ? set_free(s, s->rows) : DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_microfacet_set_eval_batch(djb_ctx *ctx, const djb_microfacet_set *s, int64_t n, const int32_t *material, const djb_vec3_view *i,
                                         const djb_vec3_view *o, int want, const djb_vec3_view *out_fr, float *out_pdf, int mem)
try {
	djb_status st = set_check(ctx, s, "microfacet");
	if (st != DJB_OK) return st;
	if (want != 1 && want != 2 && want != 4 && want != 5 && want != 6)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: want must be 1 (eval) or 2 (evalp), optionally | 4 (pdf), or 4 alone (got %d)", want);
	if (is_cpu(ctx)) return djbcpu::microfacet_set_eval(ctx, s->kind, s->rows, s->n_mat, n, material, i, o, want, out_fr, out_pdf);
	if ((want & 3) && !Staged::valid(out_fr)) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null output vec3 view");
	if ((want & 4) && !out_pdf) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null output array");
	BatchEntry c(ctx, nullptr, n, mem);
	if (c.st != DJB_OK) return c.st;
	View vi, vo, vout = { nullptr, nullptr, nullptr, 0 };
	float *dpdf = nullptr;
	if ((st = stage_material(c.sg, material, &c.dmat)) != DJB_OK) return st;
	if ((st = c.sg.in_vec(i, &vi)) != DJB_OK) return st;
	if ((st = c.sg.in_vec(o, &vo)) != DJB_OK) return st;
	if ((want & 3) && (st = c.sg.out_vec(out_fr, &vout)) != DJB_OK) return st;
	if ((want & 4) && (st = c.sg.out_arr(out_pdf, &dpdf)) != DJB_OK) return st;
	// one launch: a lane reads its hit before it writes it (index-aligned in-place views are the only supported overlap)
	HIP_TRY(djbk::launch_microfacet_set_eval(ctx->stream, s->kind, s->rows, s->n_mat, s->fr_kind, ctx->microfacet_set_rows_global != 0, n, c.dmat, vi, vo,
	                                         vout, dpdf, want));
	return c.sg.finish();
}
DJB_ABI_CATCH

djb_status djb_microfacet_set_sample_batch(djb_ctx *ctx, const djb_microfacet_set *s, int64_t n, const int32_t *material, const float *u1,
                                           const float *u2, const djb_vec3_view *o, const djb_vec3_view *out_weight, const djb_vec3_view *out_i,
                                           float *out_pdf, int mem)
try {
	djb_status st = set_check(ctx, s, "microfacet");
	if (st != DJB_OK) return st;
	const bool is = out_weight != nullptr || out_pdf != nullptr;                   // neither: sample(); else evalp_is(), which needs both
	if (is_cpu(ctx)) return djbcpu::microfacet_set_sample(ctx, s->kind, s->rows, s->n_mat, n, material, u1, u2, o, is, out_weight, out_i, out_pdf);
	if (!Staged::valid(out_i) || (is && (!Staged::valid(out_weight) || !out_pdf))) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null output");
	if (is) {
		SampleBatch c(ctx, nullptr, n, mem, material, u1, u2, o, out_i, out_weight, out_pdf);
		if (c.st != DJB_OK) return c.st;
		HIP_TRY(djbk::launch_microfacet_set_sample(ctx->stream, s->kind, s->rows, s->n_mat, s->fr_kind, ctx->microfacet_set_rows_global != 0, n, c.dmat,
		                                           c.d1, c.d2, c.vo, c.vi, &c.vw, c.dpdf));
		return c.sg.finish();
	}
	BatchEntry c(ctx, nullptr, n, mem);
	if (c.st != DJB_OK) return c.st;
	const float *d1 = nullptr, *d2 = nullptr;
	View vo, vi;
	if ((st = stage_material(c.sg, material, &c.dmat)) != DJB_OK) return st;
	if ((st = c.sg.in_f(u1, &d1)) != DJB_OK) return st;
	if ((st = c.sg.in_f(u2, &d2)) != DJB_OK) return st;
	if ((st = c.sg.in_vec(o, &vo)) != DJB_OK) return st;
	if ((st = c.sg.out_vec(out_i, &vi)) != DJB_OK) return st;
	HIP_TRY(djbk::launch_microfacet_set_sample(ctx->stream, s->kind, s->rows, s->n_mat, s->fr_kind, ctx->microfacet_set_rows_global != 0, n, c.dmat, d1, d2,
	                                           vo, vi, nullptr, nullptr));
	return c.sg.finish();
}
DJB_ABI_CATCH

} // extern "C"
