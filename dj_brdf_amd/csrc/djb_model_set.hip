// djb_model_set.hip -- the C ABI of SGD / ABC model sets (include/djb_hip.h: djb_model_set): M resident parameter rows of one kind in one
// block, evaluated per hit by material id.  Kernels: djb_kernels_model_set.hip; host loop (CPU contexts): djb_cpu.cpp; what the three kinds
// of set share: djb_set_host.hpp.  A set has no host twin: on a GPU context a host batch of any size is staged to the device.
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

} // namespace

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
	return s ? set_free(s, s->rows) : DJB_OK;
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

} // extern "C"
