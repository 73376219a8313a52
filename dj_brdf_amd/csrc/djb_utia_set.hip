// djb_utia_set.hip -- the C ABI of UTIA material sets (include/djb_hip.h: djb_utia_set): M resident UTIA record tables in one block,
// evaluated per hit by material id.  Kernels: djb_kernels_utia_set.hip; host loop (CPU contexts): djb_cpu.cpp.  A set has no host
// twin: on a GPU context a host batch of any size is staged to the device.
#include "djb_host.hpp"

using namespace djbh;

namespace {

constexpr size_t TABLE_F4 = 8 * (size_t)(UTIA_N / 3);
constexpr size_t TABLE_BYTES = sizeof(float4) * TABLE_F4;       // 10 616 832

// the set belongs to the call's context, as a djb_brdf does
djb_status set_check(const djb_ctx *ctx, const djb_utia_set *s)
{
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null utia set");
	if (!ctx) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null ctx");
	if (is_cpu(ctx) != (s->device < 0))
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: utia set and ctx belong to different back ends (CPU / GPU)");
	if (s->ctx != ctx) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the utia set belongs to another context");
	return DJB_OK;
}

} // namespace

extern "C" {

djb_status djb_utia_set_create(djb_ctx *ctx, int n_materials, const djb_brdf *const *utias, djb_utia_set **out)
try {
	if (!ctx || !out || !utias) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	if (n_materials < 1 || n_materials > DJB_UTIA_SET_MAX)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a utia set holds 1 .. %d materials (got %d)", DJB_UTIA_SET_MAX, n_materials);
	const bool cpu = is_cpu(ctx);
	djb_status st;
	std::vector<const void *> src((size_t)n_materials);
	for (int m = 0; m < n_materials; ++m) {
		const djb_brdf *b = utias[m];
		if (cpu) { if ((st = djbcpu::utia_set_member(ctx, b, m, &src[m])) != DJB_OK) return st; continue; }
		if (!b) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: utia set member %d is a null brdf", m);
		if (is_cpu(b) || b->ctx != ctx || b->device != ctx->device)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: utia set member %d belongs to another context", m);
		if (b->dev.kind != DJB_KIND_UTIA || !b->dev.utia)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: utia set member %d is not a utia brdf (kind %d)", m, b->dev.kind);
		src[m] = b->dev.utia;
	}
	djb_utia_set *s = new djb_utia_set();
	s->device = cpu ? -1 : ctx->device;
	s->ctx = ctx;
	s->n_mat = n_materials;
	const size_t bytes = TABLE_BYTES * (size_t)n_materials;
	if (cpu) {
		s->tab = (float4 *)malloc(bytes);
		if (!s->tab) { djb_utia_set_destroy(s); return fail(DJB_ERR_OUT_OF_MEMORY, "djb_error: out of host memory (utia set of %d tables)", n_materials); }
		for (int m = 0; m < n_materials; ++m) memcpy(s->tab + (size_t)m * TABLE_F4, src[m], TABLE_BYTES);
	} else {
		if ((st = check_call(ctx, nullptr, 0, DJB_MEM_DEVICE)) != DJB_OK) { delete s; return st; }
		std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
		hipError_t e = hipMalloc((void **)&s->tab, bytes);
		for (int m = 0; m < n_materials && e == hipSuccess; ++m)            // device to device, on the context's stream
			e = hipMemcpyAsync(s->tab + (size_t)m * TABLE_F4, src[m], TABLE_BYTES, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // the sources may be destroyed as soon as this returns
		if (e != hipSuccess) {
			(void)hipGetLastError();
			(void)hipStreamSynchronize(ctx->stream);
			djb_utia_set_destroy(s);
			return fail(DJB_ERR_HIP, "djb_error: HIP allocation / copy of a utia set of %d tables (%zu bytes): %s", n_materials, bytes, hipGetErrorString(e));
		}
	}
	*out = s;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_utia_set_info(const djb_utia_set *s, int *n_materials)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null utia set");
	if (n_materials) *n_materials = s->n_mat;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_utia_set_destroy(djb_utia_set *s)
try {
	if (!s) return DJB_OK;
	if (s->device < 0) free(s->tab);
	else {
		(void)hipSetDevice(s->device);
		if (s->tab) (void)hipFree(s->tab);
	}
	delete s;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_utia_set_eval_batch(djb_ctx *ctx, const djb_utia_set *s, int64_t n, const int32_t *material, const djb_vec3_view *i,
                                   const djb_vec3_view *o, int want_cos, const djb_vec3_view *out_fr, int mem)
try {
	djb_status st = set_check(ctx, s);
	if (st != DJB_OK) return st;
	if (is_cpu(ctx)) return djbcpu::utia_set_eval(ctx, s->tab, s->n_mat, n, material, i, o, want_cos, out_fr);
	if ((st = check_call(ctx, nullptr, n, mem)) != DJB_OK) return st;
	std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
	Staged sg(ctx, n, mem);
	const int32_t *dmat; View vi, vo, vout;
	if ((st = stage_material(sg, material, &dmat)) != DJB_OK) return st;
	if ((st = sg.in_vec(i, &vi)) != DJB_OK) return st;
	if ((st = sg.in_vec(o, &vo)) != DJB_OK) return st;
	if ((st = sg.out_vec(out_fr, &vout)) != DJB_OK) return st;
	// Tier 1 writes placeholders and tier 2 re-reads its inputs (worklist overflow: the whole batch), as for the single-material call
	// (djb_host_ops.hip: eval_common): a device-resident caller whose outputs overlap an input stream, the ids included, takes the
	// exact kernel alone, which reads a hit before it writes it (index-aligned in-place views are the only supported overlap)
	bool aliased = false;
	if (mem == DJB_MEM_DEVICE && n > 0) {
		auto span = [&](const void *q, long long stride) { return std::make_pair((uintptr_t)q, (uintptr_t)q + 4 * (uintptr_t)((n - 1) * stride + 1)); };
		auto hit = [&](const void *a, long long sa, const void *bq, long long sb) {
			auto x = span(a, sa), y = span(bq, sb);
			return x.first < y.second && y.first < x.second;
		};
		const void *ins[7] = { vi.x, vi.y, vi.z, vo.x, vo.y, vo.z, dmat };
		const long long sin_[7] = { vi.stride, vi.stride, vi.stride, vo.stride, vo.stride, vo.stride, 1 };
		const float *outs_[3] = { vout.x, vout.y, vout.z };
		for (int a = 0; a < 3 && !aliased; ++a) for (int c = 0; c < 7; ++c) if (hit(outs_[a], vout.stride, ins[c], sin_[c])) { aliased = true; break; }
	}
	const bool exact_only = ctx->utia_exact_only != 0 || aliased;
	// hit indices travel as uint32, so very large batches are chunked; the worklist (16-byte header + 4 bytes per entry) shares the
	// context's scratch and is sized as the single-material call sizes it
	const long long CH = 1LL << 31;
	for (long long lo = 0; lo < n; lo += CH) {
		const long long m = n - lo < CH ? n - lo : CH;
		unsigned int *count = nullptr, *list = nullptr;
		size_t cap = 0;
		if (!exact_only) {
			cap = (size_t)(m / 256 + 4096);
			if (ctx->test_worklist_cap >= 0) cap = (size_t)ctx->test_worklist_cap;   // DJB_OPT_TEST_WORKLIST_CAP (tests): force the overflow path
			const size_t need = 16 + 4 * (cap ? cap : 1);
			if (ctx->scratch_bytes < need) {
				HIP_TRY(hipStreamSynchronize(ctx->stream));
				if (ctx->scratch) (void)hipFree(ctx->scratch);
				ctx->scratch = nullptr; ctx->scratch_bytes = 0;
				HIP_TRY(hipMalloc(&ctx->scratch, need));
				ctx->scratch_bytes = need;
			}
			count = (unsigned int *)ctx->scratch; list = count + 4;
		}
		auto off = [&](const View &v) { return View{ v.x + lo * v.stride, v.y + lo * v.stride, v.z + lo * v.stride, v.stride }; };
		HIP_TRY(djbk::launch_utia_set_eval(ctx->stream, s->tab, s->n_mat, m, dmat + lo, off(vi), off(vo), off(vout), want_cos != 0, list,
		                                   (unsigned int)cap, count, exact_only));
	}
	return sg.finish();
}
DJB_ABI_CATCH

} // extern "C"
