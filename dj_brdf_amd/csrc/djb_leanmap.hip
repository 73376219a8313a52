// djb_leanmap.hip -- resident LEAN maps: the gfx950 builder / lookup kernels and the djb_leanmap entry points of include/djb_hip.h
// (the fused per-hit calls, djb_eval_leanmap_batch / djb_sample_leanmap_batch, are in djb_host_ops.hip next to the per-pair
// entries they extend).  The per-texel code is djb_leanmap.inc, shared with the host path (djb_cpu.cpp).
#include "djb_host.hpp"

using namespace djbh;
using namespace djbdev;

// ------------------------------------------------------------------ kernels: one thread per texel / per hit, nothing to tune --
// every builder moves each byte once
namespace {
constexpr int LBLOCK = 256;
inline int lgrid(long long n) { long long b = (n + LBLOCK - 1) / LBLOCK; return (int)(b < 1 ? 1 : b > 65536 ? 65536 : b); }

__global__ __launch_bounds__(LBLOCK) void k_dmap_to_nmap(int w, int h, const unsigned char *dmap, float scale, unsigned char *rgb)
{
	const long long n = (long long)w * h, stride = (long long)gridDim.x * LBLOCK;
	for (long long k = (long long)blockIdx.x * LBLOCK + threadIdx.x; k < n; k += stride)
		dmap_to_nmap_texel(dmap, w, h, (int)(k % w), (int)(k / w), scale, rgb + 3 * k);
}

__global__ __launch_bounds__(LBLOCK) void k_leanmap_from_nmap(long long n, const unsigned char *rgb, int pixel_stride, float base_roughness,
                                                              float4 *level0)
{
	const long long stride = (long long)gridDim.x * LBLOCK;
	for (long long k = (long long)blockIdx.x * LBLOCK + threadIdx.x; k < n; k += stride) {
		const unsigned char *px = rgb + (long long)pixel_stride * k;
		float e[5];
		nmap_to_lean_texel(px[0], px[1], px[2], base_roughness, e);
		leanmap_store(level0 + 2 * k, e);
	}
}

__global__ __launch_bounds__(LBLOCK) void k_leanmap_from_moments(long long n, const float *moments5, int biased, float4 *level0)
{
	const long long stride = (long long)gridDim.x * LBLOCK;
	for (long long k = (long long)blockIdx.x * LBLOCK + threadIdx.x; k < n; k += stride) {
		float e[5];
		for (int c = 0; c < 5; ++c) e[c] = moments5[5 * k + c];
		if (biased) { e[0] -= 25.0f; e[1] -= 25.0f; e[4] -= 625.0f; }
		leanmap_store(level0 + 2 * k, e);
	}
}

__global__ __launch_bounds__(LBLOCK) void k_leanmap_downsample(const float4 *src, int ws, int hs, float4 *dst, int wd, int hd)
{
	const long long n = (long long)wd * hd, stride = (long long)gridDim.x * LBLOCK;
	for (long long k = (long long)blockIdx.x * LBLOCK + threadIdx.x; k < n; k += stride) {
		float e[5];
		leanmap_downsample_texel(src, ws, hs, (int)(k % wd), (int)(k / wd), e);
		leanmap_store(dst + 2 * k, e);
	}
}

__global__ __launch_bounds__(LBLOCK) void k_leanmap_lookup(LeanSrc src, long long n, float *out5)
{
	const long long stride = (long long)gridDim.x * LBLOCK;
	for (long long k = (long long)blockIdx.x * LBLOCK + threadIdx.x; k < n; k += stride) {
		float r[5];
		leanmap_lookup_hit(src, k, r);
		for (int c = 0; c < 5; ++c) out5[5 * k + c] = r[c];
	}
}
} // namespace

namespace djbk {
hipError_t launch_dmap_to_nmap(hipStream_t s, int w, int h, const unsigned char *dmap, float scale, unsigned char *rgb)
{
	hipLaunchKernelGGL(k_dmap_to_nmap, dim3(lgrid((long long)w * h)), dim3(LBLOCK), 0, s, w, h, dmap, scale, rgb);
	return hipGetLastError();
}
hipError_t launch_leanmap_from_nmap(hipStream_t s, int w, int h, const unsigned char *rgb, int pixel_stride, float base_roughness, float4 *level0)
{
	const long long n = (long long)w * h;
	hipLaunchKernelGGL(k_leanmap_from_nmap, dim3(lgrid(n)), dim3(LBLOCK), 0, s, n, rgb, pixel_stride, base_roughness, level0);
	return hipGetLastError();
}
hipError_t launch_leanmap_from_moments(hipStream_t s, int w, int h, const float *moments5, int biased, float4 *level0)
{
	const long long n = (long long)w * h;
	hipLaunchKernelGGL(k_leanmap_from_moments, dim3(lgrid(n)), dim3(LBLOCK), 0, s, n, moments5, biased, level0);
	return hipGetLastError();
}
hipError_t launch_leanmap_downsample(hipStream_t s, const float4 *src, int ws, int hs, float4 *dst, int wd, int hd)
{
	hipLaunchKernelGGL(k_leanmap_downsample, dim3(lgrid((long long)wd * hd)), dim3(LBLOCK), 0, s, src, ws, hs, dst, wd, hd);
	return hipGetLastError();
}
hipError_t launch_leanmap_lookup(hipStream_t s, const LeanSrc &src, long long n, float *out5)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_leanmap_lookup, dim3(lgrid(n)), dim3(LBLOCK), 0, s, src, n, out5);
	return hipGetLastError();
}
} // namespace djbk

// ------------------------------------------------------------------ the handle
namespace djbh {
static int log2_exact(int v)
{
	if (v < 1 || v > (1 << LEANMAP_MAX_LOG2) || (v & (v - 1))) return -1;
	int l = 0;
	while ((1 << l) < v) ++l;
	return l;
}
static djb_status leanmap_dims(int w, int h, int *lw, int *lh)
{
	*lw = log2_exact(w); *lh = log2_exact(h);
	if (*lw < 0 || *lh < 0)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a LEAN map is 2^a x 2^b texels, 1 .. %d each (got %d x %d)", 1 << LEANMAP_MAX_LOG2, w, h);
	return DJB_OK;
}

// the map must belong to the context, as a djb_brdf must (cpu_pair_check / check_call)
djb_status leanmap_check(const djb_ctx *ctx, const djb_leanmap *m)
{
	if (!ctx) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null ctx");
	if (!m) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null leanmap");
	if (is_cpu(ctx) != (m->device < 0))
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: leanmap and ctx belong to different back ends (CPU / GPU)");
	if (!is_cpu(ctx) && m->device != ctx->device)
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: leanmap lives on device %d, ctx on %d", m->device, ctx->device);
	return DJB_OK;
}

// the host copy of a GPU map, for the host twin (scalar-size DJB_MEM_HOST calls): made by the first such call.  The map is
// immutable and complete (its stream was synchronised) since its constructor returned, so a blocking copy is all it takes.
djb_status leanmap_host_texels(const djb_leanmap *m, const float **out)
{
	if (m->device < 0) { *out = m->host.data(); return DJB_OK; }
	if (!m->host_ready.load(std::memory_order_acquire)) {
		std::lock_guard<std::mutex> g(m->host_mu);
		if (!m->host_ready.load(std::memory_order_relaxed)) {
			const size_t count = (size_t)leanmap_total_texels(m->lw, m->lh) * 8;
			m->host.resize(count);
			HIP_TRY(hipSetDevice(m->device));
			HIP_TRY(hipMemcpy(m->host.data(), m->dev, count * sizeof(float), hipMemcpyDeviceToHost));
			m->host_ready.store(1, std::memory_order_release);
		}
	}
	*out = m->host.data();
	return DJB_OK;
}

// a device buffer that lives for one constructor call
struct TmpDev {
	void *p = nullptr;
	~TmpDev() { if (p) (void)hipFree(p); }
	djb_status upload(const void *host, size_t bytes)
	{
		HIP_TRY(hipMalloc(&p, bytes ? bytes : 4));
		if (bytes) HIP_TRY(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
		return DJB_OK;
	}
	djb_status alloc(size_t bytes) { HIP_TRY(hipMalloc(&p, bytes ? bytes : 4)); return DJB_OK; }
};

static djb_status leanmap_alloc(djb_ctx *ctx, int lw, int lh, djb_leanmap **out)
{
	djb_leanmap *m = new djb_leanmap();
	m->device = is_cpu(ctx) ? -1 : ctx->device;
	m->lw = lw; m->lh = lh;
	const size_t count = (size_t)leanmap_total_texels(lw, lh) * 8;
	if (is_cpu(ctx)) m->host.assign(count, 0.0f);
	else {
		hipError_t e = hipMalloc((void **)&m->dev, count * sizeof(float));
		if (e != hipSuccess) { (void)hipGetLastError(); delete m; return fail(DJB_ERR_HIP, "djb_error: HIP hipMalloc of a LEAN map (%zu bytes): %s", count * sizeof(float), hipGetErrorString(e)); }
	}
	*out = m;
	return DJB_OK;
}

// levels 1 .. top from level 0, on the map's own back end; a GPU map is complete when this returns
static djb_status leanmap_finish(djb_ctx *ctx, djb_leanmap *m)
{
	if (m->device < 0) { djbcpu::leanmap_build_pyramid(ctx, m->lw, m->lh, m->host.data()); return DJB_OK; }
	const int levels = leanmap_levels(m->lw, m->lh);
	for (int l = 1; l < levels; ++l) {
		const int ws = 1 << (m->lw > l - 1 ? m->lw - (l - 1) : 0), hs = 1 << (m->lh > l - 1 ? m->lh - (l - 1) : 0);
		const int wd = 1 << (m->lw > l ? m->lw - l : 0), hd = 1 << (m->lh > l ? m->lh - l : 0);
		HIP_TRY(djbk::launch_leanmap_downsample(ctx->stream, m->dev + 2ull * leanmap_level_offset(m->lw, m->lh, l - 1), ws, hs,
		                                        m->dev + 2ull * leanmap_level_offset(m->lw, m->lh, l), wd, hd));
	}
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return DJB_OK;
}

// create_from_nmap / create_from_dmap share everything but where the normal map comes from
static djb_status leanmap_create_common(djb_ctx *ctx, int w, int h, const unsigned char *dmap, float scale, const unsigned char *rgb,
                                        int pixel_stride, float base_roughness, djb_leanmap **out)
{
	if (!ctx || !out || (!dmap && !rgb)) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	int lw, lh;
	djb_status st = leanmap_dims(w, h, &lw, &lh);
	if (st != DJB_OK) return st;
	if (rgb && pixel_stride < 3) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: a normal map has at least 3 bytes per pixel (pixel_stride %d)", pixel_stride);
	const size_t n = (size_t)w * h;
	djb_leanmap *m = nullptr;
	if (is_cpu(ctx)) {
		if ((st = leanmap_alloc(ctx, lw, lh, &m)) != DJB_OK) return st;
		std::vector<unsigned char> tmp;
		if (dmap) { tmp.resize(3 * n); djbcpu::dmap_to_nmap(ctx, w, h, dmap, scale, tmp.data()); rgb = tmp.data(); pixel_stride = 3; }
		djbcpu::leanmap_level0_from_nmap(ctx, w, h, rgb, pixel_stride, base_roughness, m->host.data());
	} else {
		if ((st = check_call(ctx, nullptr, 0, DJB_MEM_HOST)) != DJB_OK) return st;
		std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
		if ((st = leanmap_alloc(ctx, lw, lh, &m)) != DJB_OK) return st;
		TmpDev src, nm;
		const unsigned char *drgb;
		if (dmap) {                       // the normal map never leaves the device
			if ((st = src.upload(dmap, n)) != DJB_OK || (st = nm.alloc(3 * n)) != DJB_OK) { djb_leanmap_destroy(m); return st; }
			hipError_t e = djbk::launch_dmap_to_nmap(ctx->stream, w, h, (const unsigned char *)src.p, scale, (unsigned char *)nm.p);
			if (e != hipSuccess) { djb_leanmap_destroy(m); return fail(DJB_ERR_HIP, "djb_error: HIP launch of the normal-map kernel: %s", hipGetErrorString(e)); }
			drgb = (const unsigned char *)nm.p; pixel_stride = 3;
		} else {
			if ((st = src.upload(rgb, n * (size_t)pixel_stride)) != DJB_OK) { djb_leanmap_destroy(m); return st; }
			drgb = (const unsigned char *)src.p;
		}
		hipError_t e = djbk::launch_leanmap_from_nmap(ctx->stream, w, h, drgb, pixel_stride, base_roughness, m->dev);
		if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); djb_leanmap_destroy(m); return fail(DJB_ERR_HIP, "djb_error: HIP launch of the LEAN level-0 kernel: %s", hipGetErrorString(e)); }
		if ((st = leanmap_finish(ctx, m)) != DJB_OK) { (void)hipStreamSynchronize(ctx->stream); djb_leanmap_destroy(m); return st; }
		*out = m;
		return DJB_OK;                    // the temporaries go after the stream was synchronised by leanmap_finish
	}
	if ((st = leanmap_finish(ctx, m)) != DJB_OK) { djb_leanmap_destroy(m); return st; }
	*out = m;
	return DJB_OK;
}
} // namespace djbh

// ------------------------------------------------------------------ C ABI
djb_status djb_dmap_to_nmap(djb_ctx *ctx, int w, int h, const unsigned char *dmap, float scale, unsigned char *out_rgb)
try {
	if (!ctx || !dmap || !out_rgb) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	int lw, lh;
	djb_status st = leanmap_dims(w, h, &lw, &lh);
	if (st != DJB_OK) return st;
	if (is_cpu(ctx)) { djbcpu::dmap_to_nmap(ctx, w, h, dmap, scale, out_rgb); return DJB_OK; }
	if ((st = check_call(ctx, nullptr, 0, DJB_MEM_HOST)) != DJB_OK) return st;
	std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
	const size_t n = (size_t)w * h;
	TmpDev src, dst;
	if ((st = src.upload(dmap, n)) != DJB_OK || (st = dst.alloc(3 * n)) != DJB_OK) return st;
	HIP_TRY(djbk::launch_dmap_to_nmap(ctx->stream, w, h, (const unsigned char *)src.p, scale, (unsigned char *)dst.p));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	HIP_TRY(hipMemcpy(out_rgb, dst.p, 3 * n, hipMemcpyDeviceToHost));
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_leanmap_create_from_nmap(djb_ctx *ctx, int w, int h, const unsigned char *rgb, int pixel_stride, float base_roughness,
                                        djb_leanmap **out)
try {
	if (!rgb) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	return leanmap_create_common(ctx, w, h, nullptr, 0.0f, rgb, pixel_stride, base_roughness, out);
}
DJB_ABI_CATCH

djb_status djb_leanmap_create_from_dmap(djb_ctx *ctx, int w, int h, const unsigned char *dmap, float scale, float base_roughness,
                                        djb_leanmap **out)
try {
	if (!dmap) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	return leanmap_create_common(ctx, w, h, dmap, scale, nullptr, 3, base_roughness, out);
}
DJB_ABI_CATCH

djb_status djb_leanmap_create_from_moments(djb_ctx *ctx, int w, int h, const float *moments, int biased, djb_leanmap **out)
try {
	if (!ctx || !out || !moments) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	*out = nullptr;
	int lw, lh;
	djb_status st = leanmap_dims(w, h, &lw, &lh);
	if (st != DJB_OK) return st;
	djb_leanmap *m = nullptr;
	if (is_cpu(ctx)) {
		if ((st = leanmap_alloc(ctx, lw, lh, &m)) != DJB_OK) return st;
		djbcpu::leanmap_level0_from_moments(ctx, w, h, moments, biased != 0, m->host.data());
		if ((st = leanmap_finish(ctx, m)) != DJB_OK) { djb_leanmap_destroy(m); return st; }
		*out = m;
		return DJB_OK;
	}
	if ((st = check_call(ctx, nullptr, 0, DJB_MEM_HOST)) != DJB_OK) return st;
	std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
	if ((st = leanmap_alloc(ctx, lw, lh, &m)) != DJB_OK) return st;
	TmpDev src;
	if ((st = src.upload(moments, sizeof(float) * 5 * (size_t)w * h)) != DJB_OK) { djb_leanmap_destroy(m); return st; }
	hipError_t e = djbk::launch_leanmap_from_moments(ctx->stream, w, h, (const float *)src.p, biased != 0, m->dev);
	if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); djb_leanmap_destroy(m); return fail(DJB_ERR_HIP, "djb_error: HIP launch of the LEAN import kernel: %s", hipGetErrorString(e)); }
	if ((st = leanmap_finish(ctx, m)) != DJB_OK) { (void)hipStreamSynchronize(ctx->stream); djb_leanmap_destroy(m); return st; }
	*out = m;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_leanmap_info(const djb_leanmap *m, int *w, int *h, int *levels)
try {
	if (!m) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null leanmap");
	if (w) *w = 1 << m->lw;
	if (h) *h = 1 << m->lh;
	if (levels) *levels = leanmap_levels(m->lw, m->lh);
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_leanmap_get_level(const djb_leanmap *m, int level, int biased, float *out)
try {
	if (!m || !out) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	if (level < 0 || level >= leanmap_levels(m->lw, m->lh))
		return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: the LEAN map has levels 0 .. %d (got %d)", leanmap_levels(m->lw, m->lh) - 1, level);
	const size_t n = (size_t)1 << ((m->lw > level ? m->lw - level : 0) + (m->lh > level ? m->lh - level : 0));
	const size_t off = (size_t)leanmap_level_offset(m->lw, m->lh, level) * 8;
	std::vector<float> tmp;
	const float *t;
	if (m->device < 0) t = m->host.data() + off;
	else {
		tmp.resize(8 * n);
		HIP_TRY(hipSetDevice(m->device));
		HIP_TRY(hipMemcpy(tmp.data(), (const float *)m->dev + off, 8 * n * sizeof(float), hipMemcpyDeviceToHost));
		t = tmp.data();
	}
	for (size_t k = 0; k < n; ++k) {
		for (int c = 0; c < 5; ++c) out[5 * k + c] = t[8 * k + c];
		if (biased) { out[5 * k] += 25.0f; out[5 * k + 1] += 25.0f; out[5 * k + 4] += 625.0f; }   // nmap2leanmap_biased.cpp:54-60
	}
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_leanmap_destroy(djb_leanmap *m)
try {
	if (!m) return DJB_OK;
	if (m->dev) { (void)hipSetDevice(m->device); (void)hipFree(m->dev); }
	delete m;
	return DJB_OK;
}
DJB_ABI_CATCH

djb_status djb_leanmap_lookup_batch(djb_ctx *ctx, const djb_leanmap *m, int64_t n, const float *uv, const float *lod, float *out_lean, int mem)
try {
	djb_status st = leanmap_check(ctx, m);
	if (st != DJB_OK) return st;
	if (!uv || !out_lean) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: null argument");
	if (n < 0) return fail(DJB_ERR_INVALID_ARGUMENT, "djb_error: negative batch size");
	const bool twin = !is_cpu(ctx) && mem == DJB_MEM_HOST && n <= ctx->host_batch_max && !ctx->scalar_on_device;
	if (is_cpu(ctx) || twin) {
		const float *texels;
		if ((st = leanmap_host_texels(m, &texels)) != DJB_OK) return st;
		djbcpu::leanmap_lookup(is_cpu(ctx) ? ctx : djbcpu::twin_ctx(), texels, m->lw, m->lh, n, uv, lod, out_lean);
		return DJB_OK;
	}
	if ((st = check_call(ctx, nullptr, n, mem)) != DJB_OK) return st;
	std::lock_guard<std::recursive_mutex> call_lock(ctx->call_mu);
	Staged sg(ctx, n, mem);
	LeanSrc src{ { m->dev, m->lw, m->lh }, uv, lod };
	float *dout = nullptr;
	if ((st = stage_leanmap_coords(sg, uv, lod, &src)) != DJB_OK) return st;
	if (mem == DJB_MEM_DEVICE) dout = out_lean;
	else {
		if ((st = sg.alloc(sizeof(float) * 5 * (size_t)n, (void **)&dout)) != DJB_OK) return st;
		sg.out_raw.push_back({ dout, { out_lean, sizeof(float) * 5 * (size_t)n } });
	}
	HIP_TRY(djbk::launch_leanmap_lookup(ctx->stream, src, n, dout));
	return sg.finish();
}
DJB_ABI_CATCH
