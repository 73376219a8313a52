// djb_model_set.hip -- the C ABI of SGD / ABC model sets (include/djb_hip.h: djb_model_set): M resident parameter rows of one kind in one
// block, evaluated per hit by material id.  Kernels: djb_kernels_model_set.hip; host loop (CPU contexts): djb_cpu.cpp.  A set has no host
// twin: on a GPU context a host batch of any size is staged to the device.
#include "djb_host.hpp"

using namespace djbh;

namespace {

int row_doubles(int kind) { return kind == DJB_KIND_SGD ? 33 : 9; }

// the set belongs to the call's context, as a djb_brdf does
djb_status set_check(const djb_ctx *ctx, const djb_model_set *s)
{
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null model set");
	if (!ctx) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null ctx");
	if (is_cpu(ctx) != (s->device < 0))
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: model set and ctx belong to different back ends (CPU / GPU)");
	if (s->ctx != ctx) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the model set belongs to another context");
	return DJB_OK;
}

// rows: n_materials x row_doubles(kind), host memory, already checked
djb_status create(djb_ctx *ctx, int kind, int n_materials, const double *rows, djb_model_set **out)
{
	const bool cpu = is_cpu(ctx);
	const int nrow = row_doubles(kind);
	djb_model_set *s = new djb_model_set();
	s->device = cpu ? -1 : ctx->device;
	s->ctx = ctx;
	s->kind = kind;
	s->n_mat = n_materials;
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
	djb_status st;
	if ((st = check_call(ctx, nullptr, 0, DJB_MEM_DEVICE)) != DJB_OK) { delete s; return st; }
	std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
	const size_t bytes = sizeof(double) * block.size();
	hipError_t e = hipMalloc((void **)&s->rows, bytes);
	if (e == hipSuccess) e = hipMemcpy(s->rows, block.data(), bytes, hipMemcpyHostToDevice);     // synchronous: `block` goes out of scope
	if (e != hipSuccess) {
		(void)hipGetLastError();
		djb_model_set_destroy(s);
		return fail(DJB_ERR_HIP, "djb_error: HIP allocation / copy of a model set of %d rows (%zu bytes): %s", n_materials, bytes, hipGetErrorString(e));
	}
	*out = s;
	return DJB_OK;
}

djb_status count_check(int n_materials)
{
	if (n_materials < 1 || n_materials > DJB_MODEL_SET_MAX)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a model set holds 1 .. %d materials (got %d)", DJB_MODEL_SET_MAX, n_materials);
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
	djb_status st = count_check(n_materials);
	if (st != DJB_OK) return st;
	return create(ctx, kind, n_materials, rows, out);
}
DJB_ABI_CATCH

djb_status djb_model_set_create_from_brdfs(djb_ctx *ctx, int n_materials, const djb_brdf *const *members, djb_model_set **out)
try {
	if (!ctx || !out || !members) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	djb_status st = count_check(n_materials);
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
			if (!b) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: model set member %d is a null brdf", m);
			if (is_cpu(b) || b->ctx != ctx || b->device != ctx->device)
				return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: model set member %d belongs to another context", m);
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
	if (!s) return DJB_OK;
	if (s->device < 0) free(s->rows);
	else {
		(void)hipSetDevice(s->device);
		if (s->rows) (void)hipFree(s->rows);
	}
	delete s;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_model_set_eval_batch(djb_ctx *ctx, const djb_model_set *s, int64_t n, const int32_t *material, const djb_vec3_view *i,
                                    const djb_vec3_view *o, int want_cos, const djb_vec3_view *out_fr, int mem)
try {
	djb_status st = set_check(ctx, s);
	if (st != DJB_OK) return st;
	if (is_cpu(ctx)) return djbcpu::model_set_eval(ctx, s->kind, s->rows, s->n_mat, n, material, i, o, want_cos, out_fr);
	if ((st = check_call(ctx, nullptr, n, mem)) != DJB_OK) return st;
	std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
	Staged sg(ctx, n, mem);
	const int32_t *dmat; View vi, vo, vout;
	if ((st = stage_material(sg, material, &dmat)) != DJB_OK) return st;
	if ((st = sg.in_vec(i, &vi)) != DJB_OK) return st;
	if ((st = sg.in_vec(o, &vo)) != DJB_OK) return st;
	if ((st = sg.out_vec(out_fr, &vout)) != DJB_OK) return st;
	// one launch: a lane reads its hit before it writes it (index-aligned in-place views are the only supported overlap), the grid strides
	// over the batch in 64-bit indices
	HIP_TRY(djbk::launch_model_set_eval(ctx->stream, s->kind, s->rows, s->n_mat, ctx->model_set_rows_global != 0, n, dmat, vi, vo, vout, want_cos != 0));
	return sg.finish();
}
DJB_ABI_CATCH

} // extern "C"
