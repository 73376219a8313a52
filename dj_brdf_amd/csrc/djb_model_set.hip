// djb_model_set.hip -- the C ABI of SGD / ABC model sets (include/djb_hip.h: djb_model_set): M resident parameter rows of one kind in one
// block, evaluated per hit by material id, and -- once fitted -- the tables of each row's tabular proxy in a second block, sampled and
// light-sampled per hit.  Kernels: djb_kernels_model_set.hip, djb_kernels_model_set_proxy.hip; host loops (CPU contexts): djb_cpu.cpp; what
// the three kinds of set share: djb_set_host.hpp.  A set has no host twin: on a GPU context a host batch of any size is staged to the device.
#include "djb_set_host.hpp"

using namespace djbh;

namespace {

int row_doubles(int kind) { return kind == DJB_KIND_SGD ? 33 : 9; }

// rows: n_materials x row_doubles(kind), host memory, already checked
djb_status create(djb_ctx *ctx, int kind, int n_materials, const double *rows, djb_model_set **out)
{
	const bool cpu = is_cpu(ctx);
	const int nrow = row_doubles(kind);
	djb_model_set *s = set_new<djb_model_set>(ctx, n_materials);
	s->kind = kind;
	if (cpu) {
		const size_t bytes = sizeof(double) * (size_t)nrow * (size_t)n_materials;
		s->rows = (double *)malloc(bytes);
		if (!s->rows) { djb_model_set_destroy(s); return fail(DJB_ERR_OUT_OF_MEMORY, "djb_error: out of host memory (model set of %d rows)", n_materials); }
		memcpy(s->rows, rows, bytes);
		*out = s;
		return DJB_OK;
	}
	// the resident block: every row as create_model builds the single one (djb_host.hip).  sgd: the 33 doubles, then the constants of the
	// decided fast tier (sgd_fast_row; [33] = 0 for a row outside that tier's domain, and for every row under DJB_SGD_FAST=0); abc: the 9 doubles
	const int stride = djbk::model_set_row_stride(kind);
	std::vector<double> block((size_t)stride * (size_t)n_materials);
	const char *ev = getenv("DJB_SGD_FAST");
	const bool exact_only = ev && ev[0] == '0';
	for (int m = 0; m < n_materials; ++m) {
		double *dst = block.data() + (size_t)m * stride;
		const double *row = rows + (size_t)m * nrow;
		if (kind == DJB_KIND_SGD) {
			(void)djbdev::sgd_fast_row(row, dst);
			if (exact_only) dst[djbdev::SGD_FAST_FLAG] = 0.0;
		} else memcpy(dst, row, sizeof(double) * (size_t)nrow);
	}
	const size_t bytes = sizeof(double) * block.size();
	djb_status st = set_gpu_fill(s, djb_model_set_destroy, "model", n_materials, "rows", bytes, [&] {
		hipError_t e = hipMalloc((void **)&s->rows, bytes);
		return e == hipSuccess ? hipMemcpy(s->rows, block.data(), bytes, hipMemcpyHostToDevice) : e;     // synchronous: `block` goes out of scope
	});
	if (st != DJB_OK) return st;
	*out = s;
	return DJB_OK;
}

// the proxy block of M materials at resolution res: float[M][3][res], then int n_qf[M]
size_t proxy_floats(int n_mat, int res) { return 3 * (size_t)n_mat * (size_t)res + (size_t)n_mat; }

// A GPU set's fit.  The device views are built straight onto the resident rows -- the block holds each row as create_model builds the
// single one -- with create_model's Fresnel operands, read from a host copy of the block.  launch_fit runs on chunks of FIT_CHUNK = 128
// materials: with fit_parts that is one workgroup per CU of a 256-CU device, and it bounds the fitter's work arrays (km: n * parts *
// (res - 1)^2 doubles, 16 MB per chunk at res 90 with 2 parts; the ratio scratch 12 MB), which run_fit takes from the context's staging
// pool, whatever M is.  A material's tables do not depend on the chunk it is fitted in: the fitter's workgroups share nothing across
// materials, and its slices (fit_parts) are value-neutral.
constexpr int FIT_CHUNK = 128;
djb_status fit_gpu(djb_ctx *ctx, const djb_model_set *s, int res, int shadow, std::vector<float> *block)
{
	const int M = s->n_mat, stride = djbk::model_set_row_stride(s->kind);
	std::vector<double> rows((size_t)stride * (size_t)M);
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	HIP_TRY(hipMemcpy(rows.data(), s->rows, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
	std::vector<float> p22, sigma, qf;
	std::vector<int> n_qf;
	int *n_qf_out = (int *)(block->data() + 3 * (size_t)M * (size_t)res);
	for (int m0 = 0; m0 < M; m0 += FIT_CHUNK) {
		const int cnt = std::min(FIT_CHUNK, M - m0);
		std::vector<Brdf> srcs((size_t)cnt);
		for (int c = 0; c < cnt; ++c) {
			Brdf &b = srcs[c];
			const double *row = rows.data() + (size_t)(m0 + c) * stride;
			memset(&b, 0, sizeof b);
			b.kind = s->kind; b.shadow = 1;
			b.model = s->rows + (size_t)(m0 + c) * stride;
			if (s->kind == DJB_KIND_SGD) {
				b.fr.kind = djbdev::FR_SGD;
				for (int k = 0; k < 3; ++k) { b.fr.a[k] = (float)row[12 + k]; b.fr.b[k] = (float)row[15 + k]; }
			} else {
				b.fr.kind = djbdev::FR_UNPOLARIZED;
				for (int k = 0; k < 3; ++k) b.fr.a[k] = (float)row[8];
			}
		}
		const size_t each = (size_t)cnt * (size_t)res;
		p22.resize(each); sigma.resize(each); qf.resize(each); n_qf.resize((size_t)cnt);
		djb_status st = fit_tables(ctx, srcs, s->kind, res, shadow, p22.data(), sigma.data(), qf.data(), n_qf.data());
		if (st != DJB_OK) return st;
		for (int c = 0; c < cnt; ++c) {                                               // gather: [chunk][res] per table -> [M][3][res]
			float *dst = block->data() + 3 * (size_t)(m0 + c) * (size_t)res;
			memcpy(dst, p22.data() + (size_t)c * res, sizeof(float) * (size_t)res);
			memcpy(dst + res, sigma.data() + (size_t)c * res, sizeof(float) * (size_t)res);
			memcpy(dst + 2 * (size_t)res, qf.data() + (size_t)c * res, sizeof(float) * (size_t)res);
			n_qf_out[m0 + c] = n_qf[c];
		}
	}
	return DJB_OK;
}

// the checks the two per-hit proxy calls share, before anything is written
djb_status proxy_call_check(const djb_ctx *ctx, const djb_model_set *s)
{
	djb_status st = set_check(ctx, s, "model");
	if (st != DJB_OK) return st;
	if (!s->proxy_res) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the model set has no proxy (djb_model_set_fit_proxy)");
	return DJB_OK;
}

} // namespace

static_assert(DJB_MODEL_SET_PROXY_MAX_ENTRIES == djbk::MODEL_SET_PROXY_MAX_ENTRIES, "the header states the kernels' bound");

extern "C" {

djb_status djb_model_set_create(djb_ctx *ctx, int kind, int n_materials, const double *rows, djb_model_set **out)
try {
	if (!ctx || !out || !rows) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	if (kind != DJB_KIND_SGD && kind != DJB_KIND_ABC)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a model set is of kind sgd (%d) or abc (%d) (got %d)", DJB_KIND_SGD, DJB_KIND_ABC, kind);
	djb_status st = set_count_check("model", n_materials, DJB_MODEL_SET_MAX);
	if (st != DJB_OK) return st;
	return create(ctx, kind, n_materials, rows, out);
}
DJB_ABI_CATCH

djb_status djb_model_set_create_from_brdfs(djb_ctx *ctx, int n_materials, const djb_brdf *const *members, djb_model_set **out)
try {
	if (!ctx || !out || !members) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	djb_status st = set_count_check("model", n_materials, DJB_MODEL_SET_MAX);
	if (st != DJB_OK) return st;
	const bool cpu = is_cpu(ctx);
	int kind = -1;
	std::vector<double> rows;
	for (int m = 0; m < n_materials; ++m) {
		const djb_brdf *b = members[m];
		int k = -1;
		const double *row = nullptr;
		if (cpu) { if ((st = djbcpu::model_set_member(ctx, b, m, &k, &row)) != DJB_OK) return st; }
		else {
			if ((st = set_gpu_member(ctx, b, m, "model")) != DJB_OK) return st;
			k = b->dev.kind;
			if ((k != DJB_KIND_SGD && k != DJB_KIND_ABC) || b->model_host.size() != (size_t)row_doubles(k))
				return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: model set member %d is not an sgd or abc brdf (kind %d)", m, k);
			row = b->model_host.data();
		}
		if (m == 0) { kind = k; rows.reserve((size_t)row_doubles(k) * (size_t)n_materials); }
		else if (k != kind)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: model set member %d is of kind %d, member 0 of kind %d (a set holds one kind)", m, k, kind);
		rows.insert(rows.end(), row, row + row_doubles(k));
	}
	return create(ctx, kind, n_materials, rows.data(), out);
}
DJB_ABI_CATCH

djb_status djb_model_set_info(const djb_model_set *s, int *kind, int *n_materials)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null model set");
	if (kind) *kind = s->kind;
	if (n_materials) *n_materials = s->n_mat;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_model_set_destroy(djb_model_set *s)
try {
	return s ? set_free(s, s->rows, s->proxy_dev) : DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_model_set_eval_batch(djb_ctx *ctx, const djb_model_set *s, int64_t n, const int32_t *material, const djb_vec3_view *i,
                                    const djb_vec3_view *o, int want_cos, const djb_vec3_view *out_fr, int mem)
try {
	djb_status st = set_check(ctx, s, "model");
	if (st != DJB_OK) return st;
	if (is_cpu(ctx)) return djbcpu::model_set_eval(ctx, s->kind, s->rows, s->n_mat, n, material, i, o, want_cos, out_fr);
	SetBatch c(ctx, nullptr, n, mem, material, i, o, out_fr);
	if (c.st != DJB_OK) return c.st;
	// one launch: a lane reads its hit before it writes it (index-aligned in-place views are the only supported overlap), the grid strides
	// over the batch in 64-bit indices
	HIP_TRY(djbk::launch_model_set_eval(ctx->stream, s->kind, s->rows, s->n_mat, ctx->model_set_rows_global != 0, n, c.dmat, c.vi, c.vo, c.vout,
	                                    want_cos != 0));
	return c.sg.finish();
}
DJB_ABI_CATCH

djb_status djb_model_set_fit_proxy(djb_ctx *ctx, djb_model_set *s, int res, int shadow)
try {
	djb_status st = set_check(ctx, s, "model");
	if (st != DJB_OK) return st;
	if (res <= 2) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: Invalid Resolution");                   // dj_brdf.h:2218
	if ((long long)s->n_mat * res > DJB_MODEL_SET_PROXY_MAX_ENTRIES)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a model set's proxy holds at most %lld table entries per table (%d materials x resolution %d)",
		            (long long)DJB_MODEL_SET_PROXY_MAX_ENTRIES, s->n_mat, res);
	std::vector<float> block(proxy_floats(s->n_mat, res));
	if (is_cpu(ctx)) {
		if ((st = djbcpu::model_set_fit_proxy(ctx, s->kind, s->rows, s->n_mat, res, shadow, block.data())) != DJB_OK) return st;
	} else {
		if ((st = check_call(ctx, nullptr, 0, DJB_MEM_DEVICE)) != DJB_OK) return st;
		std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
		if ((st = fit_gpu(ctx, s, res, shadow, &block)) != DJB_OK) return st;
		// the new block, then -- every earlier call on the stream has finished with the old one -- the exchange
		float *d = nullptr;
		const size_t bytes = sizeof(float) * block.size();
		hipError_t e = hipMalloc((void **)&d, bytes);
		if (e == hipSuccess) e = hipMemcpyAsync(d, block.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) {
			(void)hipGetLastError();
			if (d) (void)hipFree(d);
			return fail(DJB_ERR_HIP, "djb_error: HIP allocation / copy of a model set's proxy block (%zu bytes): %s", bytes, hipGetErrorString(e));
		}
		if (s->proxy_dev) (void)hipFree(s->proxy_dev);
		s->proxy_dev = d;
	}
	s->proxy_host.swap(block);
	s->proxy_res = res; s->proxy_shadow = shadow != 0;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_model_set_proxy_info(const djb_model_set *s, int *res, int *shadow)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null model set");
	if (res) *res = s->proxy_res;
	if (shadow) *shadow = s->proxy_shadow;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_model_set_get_proxy(const djb_model_set *s, int material, int which, float *out, int *count)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null model set");
	if (!s->proxy_res) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the model set has no proxy (djb_model_set_fit_proxy)");
	if (material < 0 || material >= s->n_mat)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: material %d is outside the set's 0 .. %d", material, s->n_mat - 1);
	const size_t res = (size_t)s->proxy_res;
	const float *tab = s->proxy_host.data() + 3 * (size_t)material * res;
	int n = s->proxy_res;
	switch (which) {
	case DJB_TAB_P22: break;
	case DJB_TAB_SIGMA: tab += res; break;
	case DJB_TAB_QF: tab += 2 * res; n = ((const int *)(s->proxy_host.data() + 3 * (size_t)s->n_mat * res))[material]; break;
	default: return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a model set's proxy holds p22, sigma and qf (table %d)", which);
	}
	if (count) *count = n;
	if (out) memcpy(out, tab, sizeof(float) * (size_t)n);
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_model_set_evalp_is_proxy_batch(djb_ctx *ctx, const djb_model_set *s, int64_t n, const int32_t *material, const float *u1,
                                              const float *u2, const djb_vec3_view *o, const djb_vec3_view *out_weight,
                                              const djb_vec3_view *out_i, float *out_pdf, int mem)
try {
	djb_status st = proxy_call_check(ctx, s);
	if (st != DJB_OK) return st;
	if (is_cpu(ctx))
		return djbcpu::model_set_evalp_is_proxy(ctx, s->kind, s->rows, s->n_mat, s->proxy_host.data(), s->proxy_res, s->proxy_shadow, n, material, u1, u2,
		                                        o, out_weight, out_i, out_pdf);
	if (!Staged::valid(out_weight) || !Staged::valid(out_i) || !out_pdf) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null output");
	Params pp;
	if ((st = device_params(nullptr, &pp, DJB_KIND_TABULAR)) != DJB_OK) return st;         // as the single-material call resolves NULL proxy params
	SampleBatch c(ctx, nullptr, n, mem, material, u1, u2, o, out_i, out_weight, out_pdf);
	if (c.st != DJB_OK) return c.st;
	const djbk::ModelSetProxy px = { s->proxy_dev, s->proxy_res, s->proxy_shadow };
	HIP_TRY(djbk::launch_model_set_evalp_is_proxy(ctx->stream, s->kind, s->rows, s->n_mat, ctx->model_set_rows_global != 0, px, pp, n, c.dmat, c.d1, c.d2,
	                                              c.vo, c.vw, c.vi, c.dpdf));
	return c.sg.finish();
}
DJB_ABI_CATCH

djb_status djb_model_set_evalp_pdf_proxy_batch(djb_ctx *ctx, const djb_model_set *s, int64_t n, const int32_t *material, const djb_vec3_view *i,
                                               const djb_vec3_view *o, const djb_vec3_view *out_fr, float *out_pdf, int mem)
try {
	djb_status st = proxy_call_check(ctx, s);
	if (st != DJB_OK) return st;
	if (!out_pdf) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null out_pdf (evalp alone: djb_model_set_eval_batch)");
	if (is_cpu(ctx))
		return djbcpu::model_set_evalp_pdf(ctx, s->kind, s->rows, s->n_mat, s->proxy_host.data(), s->proxy_res, s->proxy_shadow, n, material, i, o,
		                                   out_fr, out_pdf);
	Params pp;
	if ((st = device_params(nullptr, &pp, DJB_KIND_TABULAR)) != DJB_OK) return st;
	SetBatch c(ctx, nullptr, n, mem, material, i, o, out_fr);
	if (c.st != DJB_OK) return c.st;
	float *dpdf = nullptr;
	if ((st = c.sg.out_arr(out_pdf, &dpdf)) != DJB_OK) return st;
	const djbk::ModelSetProxy px = { s->proxy_dev, s->proxy_res, s->proxy_shadow };
	HIP_TRY(djbk::launch_model_set_evalp_pdf(ctx->stream, s->kind, s->rows, s->n_mat, ctx->model_set_rows_global != 0, px, pp, n, c.dmat, c.vi, c.vo,
	                                         c.vout, dpdf));
	return c.sg.finish();
}
DJB_ABI_CATCH

} // extern "C"
