// djb_utia_set.hip -- the C ABI of UTIA material sets (include/djb_hip.h: djb_utia_set): M resident UTIA record tables in one block,
// evaluated per hit by material id, and -- once given -- one resolved proxy parameter set per material, which a scene's proxy calls read.  Kernels: djb_kernels_utia_set.hip; host loop (CPU contexts): djb_cpu.cpp; what the three kinds of
// set share: djb_set_host.hpp.  A set has no host twin: on a GPU context a host batch of any size is staged to the device.
#include "djb_set_host.hpp"

using namespace djbh;

namespace {

constexpr size_t TABLE_F4 = 8 * (size_t)(UTIA_N / 3);
constexpr size_t TABLE_BYTES = sizeof(float4) * TABLE_F4;       // 10 616 832

} // namespace

extern "C" {

djb_status djb_utia_set_create(djb_ctx *ctx, int n_materials, const djb_brdf *const *utias, djb_utia_set **out)
try {
	if (!ctx || !out || !utias) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	djb_status st = set_count_check("utia", n_materials, DJB_UTIA_SET_MAX);
	if (st != DJB_OK) return st;
	const bool cpu = is_cpu(ctx);
	std::vector<const void *> src((size_t)n_materials);
	for (int m = 0; m < n_materials; ++m) {
		const djb_brdf *b = utias[m];
		if (cpu) { if ((st = djbcpu::utia_set_member(ctx, b, m, &src[m])) != DJB_OK) return st; continue; }
		if ((st = set_gpu_member(ctx, b, m, "utia")) != DJB_OK) return st;
		if (b->dev.kind != DJB_KIND_UTIA || !b->dev.utia)
			return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: utia set member %d is not a utia brdf (kind %d)", m, b->dev.kind);
		src[m] = b->dev.utia;
	}
	djb_utia_set *s = set_new<djb_utia_set>(ctx, n_materials);
	const size_t bytes = TABLE_BYTES * (size_t)n_materials;
	if (cpu) {
		s->tab = (float4 *)malloc(bytes);
		if (!s->tab) { djb_utia_set_destroy(s); return fail(DJB_ERR_OUT_OF_MEMORY, "djb_error: out of host memory (utia set of %d tables)", n_materials); }
		for (int m = 0; m < n_materials; ++m) memcpy(s->tab + (size_t)m * TABLE_F4, src[m], TABLE_BYTES);
	} else if ((st = set_gpu_fill(s, djb_utia_set_destroy, "utia", n_materials, "tables", bytes,
	                              [&] { return set_gather(ctx, (void **)&s->tab, TABLE_BYTES, src); })) != DJB_OK) return st;
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

// The block is allocated by the first call (a new set has no proxy parameters); the resolve and the exchange are the MERL set's (djb_set_host.hpp)
djb_status djb_utia_set_set_proxy_params(djb_utia_set *s, const djb_params *proxy_params)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null utia set");
	std::vector<Params> resolved;
	djb_status st = resolve_all(s->device < 0, s->n_mat, proxy_params, &resolved, "utia");
	if (st != DJB_OK) return st;
	if (!s->params) {
		const size_t bytes = sizeof(Params) * (size_t)s->n_mat;
		if (s->device < 0) {
			s->params = (Params *)calloc((size_t)s->n_mat, sizeof(Params));
			if (!s->params) return fail(DJB_ERR_OUT_OF_MEMORY, "djb_error: out of host memory (proxy parameters of a utia set of %d tables)", s->n_mat);
		} else {
			HIP_TRY(hipSetDevice(s->device));
			std::lock_guard<std::recursive_mutex> call_lock(s->ctx->call_mu);
			HIP_TRY(hipMalloc((void **)&s->params, bytes));
		}
	}
	return install_params(s, resolved);
}
DJB_ABI_CATCH

djb_status djb_utia_set_proxy_info(const djb_utia_set *s, int *has_proxy_params)
try {
	if (!s) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null utia set");
	if (has_proxy_params) *has_proxy_params = s->has_params ? 1 : 0;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_utia_set_destroy(djb_utia_set *s)
try {
	return s ? set_free(s, s->tab, s->params) : DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_utia_set_eval_batch(djb_ctx *ctx, const djb_utia_set *s, int64_t n, const int32_t *material, const djb_vec3_view *i,
                                   const djb_vec3_view *o, int want_cos, const djb_vec3_view *out_fr, int mem)
try {
	djb_status st = set_check(ctx, s, "utia");
	if (st != DJB_OK) return st;
	if (is_cpu(ctx)) return djbcpu::utia_set_eval(ctx, s->tab, s->n_mat, n, material, i, o, want_cos, out_fr);
	SetBatch c(ctx, nullptr, n, mem, material, i, o, out_fr);
	if (c.st != DJB_OK) return c.st;
	const View &vi = c.vi, &vo = c.vo, &vout = c.vout;
	// Tier 1 writes placeholders and tier 2 re-reads its inputs (worklist overflow: the whole batch), as for the single-material call
	// (djb_host_ops.hip: eval_common): a device-resident caller whose outputs overlap an input stream, the ids included, takes the
	// exact kernel alone, which reads a hit before it writes it (index-aligned in-place views are the only supported overlap)
	const Stream ins[7] = { { vi.x, vi.stride }, { vi.y, vi.stride }, { vi.z, vi.stride }, { vo.x, vo.stride }, { vo.y, vo.stride }, { vo.z, vo.stride },
	                        { c.dmat, 1 } };
	const Stream outs[3] = { { vout.x, vout.stride }, { vout.y, vout.stride }, { vout.z, vout.stride } };
	const bool exact_only = ctx->utia_exact_only != 0 || (mem == DJB_MEM_DEVICE && outputs_overlap_inputs(n, ins, 7, outs, 3));
	// hit indices travel as uint32, so very large batches are chunked; the worklist (16-byte header + 4 bytes per entry) shares the
	// context's scratch and is sized as the single-material call sizes it
	for (long long lo = 0; lo < n; lo += CHUNK) {
		const long long m = std::min(n - lo, CHUNK);
		unsigned int *count = nullptr, *list = nullptr;
		size_t cap = 0;
		if (!exact_only) {
			cap = (size_t)(m / 256 + 4096);
			if (ctx->test_worklist_cap >= 0) cap = (size_t)ctx->test_worklist_cap;   // DJB_OPT_TEST_WORKLIST_CAP (tests): force the overflow path
			if ((st = ensure_scratch(ctx, 16 + 4 * (cap ? cap : 1))) != DJB_OK) return st;
			count = (unsigned int *)ctx->scratch; list = count + 4;
		}
		HIP_TRY(djbk::launch_utia_set_eval(ctx->stream, s->tab, s->n_mat, m, c.dmat + lo, offset_view(vi, lo), offset_view(vo, lo), offset_view(vout, lo),
		                                   want_cos != 0, list, (unsigned int)cap, count, exact_only));
	}
	return c.sg.finish();
}
DJB_ABI_CATCH

} // extern "C"
