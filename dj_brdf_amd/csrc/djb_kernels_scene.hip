// djb_kernels_scene.hip -- scenes: a batch of hits that lands on MERL, UTIA, sgd and abc materials at once, eval / evalp per hit.
//
// A scene maps a scene material id to (kind, local id) in up to four member sets through a resident slot table, one 32-bit word per slot:
// kind in the high 16 bits (0 merl, 1 utia, 2 sgd, 3 abc; anything else: a slot without material), the local id in the low 16.  A wave of
// a mixed batch holds all four kinds, so nothing here dispatches on kind per lane.  The batch is partitioned by kind on the device and
// each kind's kernel runs on a dense list of hit indices:
//   k_scene_count      per tile of TILE = 512 hits (one wave, 8 steps of 64) and kind: the number of hits
//   k_scene_scan       one workgroup: the exclusive scan of the [tiles][4] counts, kind-major -- each entry becomes the position of its
//                      tile's first hit of that kind in ONE list of n entries (merl segment, utia, sgd, abc); leaves count[4] and offset[4]
//   k_scene_scatter    every active hit writes its 32-bit index to its kind's segment: ballot + prefix popcount within the wave + the
//                      tile's offset -- a stable counting sort, no atomic; a dead hit (id outside the table, a slot without material)
//                      gets its +0 here and is never read again
// then, per member set the scene has, the member set's kernel with an indirection -- the loop runs over list positions j below count[kind]
// (read from device memory: a scalar load, workgroup-uniform), k = list[offset + j], directions and result at k, the local id from the
// slot of material[k]:
//   k_scene_merl<WANT>          k_merl_set_fast's body (merl_eval_hits, djb_merl_hits.inc): tier 1 in place, the 9-word record queue, the extra trip
//   k_scene_utia<WANT>          k_utia_set's body (djb_kernels_utia_set.hip): the per-wave LDS tile, six shuffles, six predicated LDS-direct
//                               loads; undecided hits append k to the worklist
//   k_scene_utia_fix<WANT>      k_utia_set_fix: the listed hits; the utia SEGMENT if the list overflowed; alone over the segment
//   k_scene_model<KIND, WANT>   k_model_set's body (model_eval_trip, djb_model_hits.inc): unit<KIND, WANT>, rows in dynamic LDS or global memory
// The MERL and sgd / abc bodies exist once, over a hit source (djb_hit_source.inc; here ListHits, djb_scene_part.inc); the utia kernels are
// written out.
// The per-unit functions are the ones those kernels call, so an active hit has the bits of its member set's call, which are the bits of
// the single-material call.  The grid of a per-kind kernel is sized for the chunk, an upper bound: a workgroup beyond the count leaves at
// once.  Nothing is read back to the host.  Every lane reads its hit before it writes it and kinds touch disjoint hits: index-aligned
// in-place calls are supported (the utia part then runs k_scene_utia_fix alone, whose lanes read before they write).
// Hit indices are chunk-relative and 32 bits wide: the host runs chunks of at most 2^26 hits (djb_scene.hip).
#include "djb_internal.hpp"
#include "djb_worklist.hpp"
#include <string.h>

using namespace djbdev;

namespace {

#include "djb_scene_part.inc"                                                                         // BLOCK, TILE, K_*, Hits, slot_of, kind_of, local_of, ListHits, wave_tile, scatter_hits
constexpr long long GRID_CAP_MERL = 256LL * 16;             // as k_merl_set_fast
constexpr long long GRID_CAP_UTIA = 256LL * 64;             // as k_utia_set
constexpr long long GRID_CAP_MODEL = 256LL * 16;            // as k_model_set

#include "djb_merl_hits.inc"                                // merl_set_texel, the queue record, merl_eval_hits
#include "djb_utia_hits.inc"                                // DJB_UTIA_MIN_WAVES, TABLE_F4, NO_RECORD, utia_target
#include "djb_model_hits.inc"                               // row_stride, unit, rows_lds, min_waves, ModelLaunch, model_eval_trip

// ---- the partition
__global__ __launch_bounds__(BLOCK) void k_scene_count(const unsigned int *slots, unsigned int n_slots, unsigned int m, const int32_t *mat,
                                                       unsigned int n_tiles, unsigned int *tiles)
{
	const unsigned int lane = threadIdx.x & 63u, tile = wave_tile();
	if (tile >= n_tiles) return;                                                  // wave-uniform
	unsigned int c[4] = { 0u, 0u, 0u, 0u };
	for (unsigned int s = 0; s < STEPS; ++s) {
		const unsigned int k = tile * TILE + s * 64u + lane;                       // m <= 2^26: no wrap
		unsigned int q = K_DEAD;
		if (k < m) q = kind_of(slot_of(slots, n_slots, (unsigned int)mat[k]));
#pragma unroll
		for (unsigned int u = 0; u < 4u; ++u) c[u] += (unsigned int)__popcll(__ballot(q == u));
	}
	if (lane < 4u) tiles[tile * 4u + lane] = lane == 0u ? c[0] : lane == 1u ? c[1] : lane == 2u ? c[2] : c[3];
}

constexpr int SCAN_BLOCK = 1024;
__global__ __launch_bounds__(SCAN_BLOCK) void k_scene_scan(unsigned int n_tiles, unsigned int *tiles, unsigned int *hdr)
{
	__shared__ unsigned int s_w[SCAN_BLOCK / 64][4];
	const unsigned int t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const unsigned int per = (n_tiles + (unsigned int)SCAN_BLOCK - 1u) / (unsigned int)SCAN_BLOCK;     // consecutive tiles per thread
	const unsigned int t0 = t * per < n_tiles ? t * per : n_tiles, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
	unsigned int sum[4] = { 0u, 0u, 0u, 0u };
	for (unsigned int a = t0; a < t1; ++a) {
#pragma unroll
		for (unsigned int u = 0; u < 4u; ++u) sum[u] += tiles[4u * a + u];
	}
	unsigned int inc[4];                                                           // inclusive over the wave's threads
#pragma unroll
	for (unsigned int u = 0; u < 4u; ++u) {
		unsigned int v = sum[u];
		for (unsigned int d = 1u; d < 64u; d <<= 1) { const unsigned int y = __shfl_up(v, d); if (lane >= d) v += y; }
		inc[u] = v;
		if (lane == 63u) s_w[wave][u] = v;
	}
	__syncthreads();
	unsigned int base[4], total[4];
#pragma unroll
	for (unsigned int u = 0; u < 4u; ++u) {
		unsigned int b = 0u, tot = 0u;
		for (unsigned int w = 0; w < (unsigned int)(SCAN_BLOCK / 64); ++w) { const unsigned int x = s_w[w][u]; if (w < wave) b += x; tot += x; }
		base[u] = b + inc[u] - sum[u]; total[u] = tot;
	}
	const unsigned int off[4] = { 0u, total[0], total[0] + total[1], total[0] + total[1] + total[2] };   // the segments, kind after kind
	for (unsigned int a = t0; a < t1; ++a) {
#pragma unroll
		for (unsigned int u = 0; u < 4u; ++u) { const unsigned int c = tiles[4u * a + u]; tiles[4u * a + u] = off[u] + base[u]; base[u] += c; }
	}
	if (t == 0u) {
#pragma unroll
		for (unsigned int u = 0; u < 4u; ++u) { hdr[u] = total[u]; hdr[4u + u] = off[u]; }
	}
}

__global__ __launch_bounds__(BLOCK) void k_scene_scatter(const unsigned int *slots, unsigned int n_slots, unsigned int m, const int32_t *mat,
                                                         unsigned int n_tiles, const unsigned int *tiles, unsigned int *list, View vout)
{
	scatter_hits(slots, n_slots, m, mat, n_tiles, tiles, list, [&](unsigned int k) { store3(vout, (long long)k, mk(0, 0, 0)); });
}

// ---- merl: merl_eval_hits over the list
template <int WANT>
__global__ __launch_bounds__(BLOCK) void k_scene_merl(Hits h, const MerlTexel *tex, unsigned int n_mat, View vi, View vo, View vout, MerlGuard g,
                                                      int merl_exact)
{
	__shared__ unsigned int s_q[BLOCK / 64][9][RECQ_CAP];
	merl_eval_hits<WANT>(ListHits(h, K_MERL, n_mat), s_q, tex, vi, vo, vout, g, merl_exact);
}

// ---- utia: k_utia_set over the list, written out (djb_utia_hits.inc)
template <int WANT>
__global__ __launch_bounds__(BLOCK, DJB_UTIA_MIN_WAVES) void k_scene_utia(Hits h, const float4 *tab, unsigned int n_mat, View vi, View vo, View vout,
                                                                         unsigned int *wl, unsigned int cap, unsigned int *wl_count)
{
	__shared__ float4 s_tile[BLOCK / 64][384];
	__shared__ double s_atan[16];
	const unsigned int cnt = h.hdr[K_UTIA], first = h.hdr[4 + K_UTIA];
	if (blockIdx.x * (unsigned int)BLOCK >= cnt) return;                           // workgroup-uniform, before the barrier
	const lds_f64p T = atan_tab(atan_tab_to_lds(s_atan, threadIdx.x));
	__syncthreads();
	const unsigned int stride = gridDim.x * (unsigned int)BLOCK;
	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	typedef __attribute__((address_space(3))) void lds_void;
	typedef __attribute__((address_space(1))) const void glb_void;
	float4 *tile = s_tile[wave];
	for (unsigned int j0 = blockIdx.x * (unsigned int)BLOCK; j0 < cnt; j0 += stride) {     // j0: workgroup-uniform
		const unsigned int j = j0 + t;
		const bool live = j < cnt;
		bool act = false;
		unsigned int id = 0u, k = 0u;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		if (live) {
			k = h.list[first + j];
			act = local_of(h, k, K_UTIA, n_mat, id);
			i = load3(vi, (long long)k); o = load3(vo, (long long)k);
		}
		v3 fr = mk(0, 0, 0);
		bool ok = true;
		if (__ballot(act) != 0ull) {                                               // wave-uniform
			const UtiaCells c = utia_cells_estimate(i, o);
			int e[2];
			utia_record_index(c, e);                                                // clamped for any input: inside the material's table
			unsigned int rec[2];
			rec[0] = act ? id * TABLE_F4 + 8u * (unsigned int)e[0] : NO_RECORD;
			rec[1] = act ? id * TABLE_F4 + 8u * (unsigned int)e[1] : NO_RECORD;
			float4 q[6];
			auto fetch = [&](int a) {
				unsigned int rec_src[6];                                                // the six shuffles first: one wait, not one per load
#pragma unroll
				for (unsigned int s = 0; s < 6u; ++s) {
					const unsigned int g = s * 64u + lane, r = (g * 10923u) >> 16;          // r = g / 6 for g < 384
					rec_src[s] = (unsigned int)__shfl((int)rec[a], (int)r);
				}
#pragma unroll
				for (unsigned int s = 0; s < 6u; ++s) {
					const unsigned int g = s * 64u + lane, r = (g * 10923u) >> 16, chunk = g - 6u * r;
					if (rec_src[s] != NO_RECORD) {
						// uniform base + unsigned 32-bit byte offset (up to 2.72e9): the saddr form of the load
						const char *src = (const char *)tab + (size_t)((rec_src[s] + chunk) << 4);
						__builtin_amdgcn_global_load_lds((glb_void *)src, (lds_void *)(tile + s * 64u), 16, 0, 0);
					}
				}
			};
			auto take = [&]() {
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                        // this wave's LDS-direct loads have landed
#pragma unroll
				for (unsigned int jj = 0; jj < 6u; ++jj) q[jj] = tile[lane * 6u + jj];
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                      // read before the tile is overwritten
			};
			fetch(0);
			UtiaTaps u;
			ok = utia_weights(i, o, c, u, T);                                       // under the fetch
			float acc[3] = { 0.0f, 0.0f, 0.0f };
			take();
			fetch(1);                                                               // in flight while record 0 is accumulated
			utia_accumulate(u, 0, q, acc);
			take();
			utia_accumulate(u, 1, q, acc);
			const v3 ev = utia_decode_t1(u, acc, ok);
			if (act) fr = (WANT & 2) ? scale(i.z, ev) : ev;                         // brdf::evalp, dj_brdf.h:803-806
		}
		if (live) {
			store3(vout, (long long)k, fr);
			if (__builtin_expect(act & !ok, 0)) {
				const unsigned int slot = atomicAdd(wl_count, 1u);
				if (slot < cap) wl[slot] = k;
			}
		}
	}
}

// alone: no tier 1 ran -- every hit of the utia segment, `wl_count` not read; a hit is read before it is written
template <int WANT>
__global__ __launch_bounds__(BLOCK) void k_scene_utia_fix(Hits h, Brdf b, const float4 *tab, unsigned int n_mat, View vi, View vo, View vout,
                                                          const unsigned int *wl, unsigned int cap, const unsigned int *wl_count, int alone)
{
	const unsigned int cnt = h.hdr[K_UTIA], first = h.hdr[4 + K_UTIA];
	const unsigned int c = alone ? 0u : *wl_count;
	const bool all = alone || c > cap;                                             // overflow: redo the segment
	const unsigned int m = all ? cnt : c;
	const Params none = {};
	const unsigned int stride = gridDim.x * (unsigned int)BLOCK;
	for (unsigned int j = blockIdx.x * (unsigned int)BLOCK + threadIdx.x; j < m; j += stride) {
		const unsigned int k = all ? h.list[first + j] : wl[j];
		unsigned int id;
		v3 fr = mk(0, 0, 0); float pdf = 0.0f;
		if (local_of(h, k, K_UTIA, n_mat, id)) {
			b.utia = tab + (size_t)id * (size_t)TABLE_F4;
			eval_one<KIND_UTIA, WANT>(b, none, load3(vi, (long long)k), load3(vo, (long long)k), fr, pdf);
		}
		store3(vout, (long long)k, fr);
	}
}

// ---- sgd / abc: model_eval_trip over the list
template <int KIND, int WANT>
__global__ __launch_bounds__(BLOCK, min_waves(KIND, false)) void k_scene_model(Hits h, Brdf b, const double *rows, unsigned int n_mat, int in_lds, View vi,
                                                                               View vo, View vout)
{
	__shared__ unsigned long long s_exp[256];
	__shared__ double s_pow[384];
	__shared__ double s_atan[KIND == KIND_SGD ? 16 : 1];
	extern __shared__ double s_rows[];                                            // n_mat * STRIDE doubles when in_lds, else none
	const ListHits src(h, KIND == KIND_SGD ? K_SGD : K_ABC, n_mat);
	if (src.none()) return;                                                        // workgroup-uniform, before the staging and its barrier
	b = stage<KIND, KIND == KIND_SGD>(b, s_exp, s_pow, s_atan, s_rows, rows, src.n_mat, in_lds);
	const unsigned int stride = src.stride();
	for (unsigned int j0 = src.start(); j0 < src.count(); j0 += stride)                      // j0: workgroup-uniform
		model_eval_trip<KIND, WANT>(src, j0, s_rows, b, rows, in_lds, vi, vo, vout);
}

template <int KIND, int WANT>
hipError_t launch_model(hipStream_t s, const Hits &h, const double *rows, int n_mat, bool rows_global, long long m, const View &i, const View &o,
                        const View &out)
{
	const ModelLaunch L(KIND, n_mat, rows_global, false);
	hipLaunchKernelGGL((k_scene_model<KIND, WANT>), dim3(djbk::grid_capped(m, BLOCK, GRID_CAP_MODEL)), dim3(BLOCK), L.lds, s, h, L.b, rows,
	                   (unsigned int)n_mat, L.in_lds, i, o, out);
	return hipGetLastError();
}

template <int WANT>
hipError_t launch_all(hipStream_t s, const djbk::SceneMembers &mb, const unsigned int *slots, int n_slots, long long m, const int32_t *mat,
                      const View &i, const View &o, const View &out, const djbk::SceneScratch &sc, bool merl_exact, bool utia_exact, bool rows_global)
{
	const unsigned int n_tiles = (unsigned int)djbk::scene_tiles(m);
	const dim3 part((n_tiles + BLOCK / 64 - 1) / (BLOCK / 64)), t(BLOCK);
	hipError_t e;
	if ((e = djbk::launch_scene_count_scan(s, slots, n_slots, m, mat, sc)) != hipSuccess) return e;
	hipLaunchKernelGGL(k_scene_scatter, part, t, 0, s, slots, (unsigned int)n_slots, (unsigned int)m, mat, n_tiles, sc.tiles, sc.list, out);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	const Hits h = { slots, (unsigned int)n_slots, mat, sc.hdr, sc.list };
	if (mb.merl) {
		hipLaunchKernelGGL((k_scene_merl<WANT>), dim3(djbk::grid_capped(m, BLOCK, GRID_CAP_MERL)), t, 0, s, h, mb.merl, (unsigned int)mb.n_merl, i, o, out,
		                   MERL_GUARD_DEFAULT, merl_exact ? 1 : 0);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (mb.utia) {
		const Brdf b = utia_target();
		const dim3 g(djbk::grid_capped(m, BLOCK, GRID_CAP_UTIA));
		if (utia_exact)
			hipLaunchKernelGGL((k_scene_utia_fix<WANT>), g, t, 0, s, h, b, mb.utia, (unsigned int)mb.n_utia, i, o, out, nullptr, 0u, nullptr, 1);
		else {
			if ((e = hipMemsetAsync(sc.wl_count, 0, 16, s)) != hipSuccess) return e;
			hipLaunchKernelGGL((k_scene_utia<WANT>), g, t, 0, s, h, mb.utia, (unsigned int)mb.n_utia, i, o, out, sc.wl, sc.wl_cap, sc.wl_count);
			if ((e = hipGetLastError()) != hipSuccess) return e;
			hipLaunchKernelGGL((k_scene_utia_fix<WANT>), dim3(64), t, 0, s, h, b, mb.utia, (unsigned int)mb.n_utia, i, o, out, sc.wl, sc.wl_cap, sc.wl_count, 0);
		}
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (mb.sgd && (e = launch_model<KIND_SGD, WANT>(s, h, mb.sgd, mb.n_sgd, rows_global, m, i, o, out)) != hipSuccess) return e;
	if (mb.abc && (e = launch_model<KIND_ABC, WANT>(s, h, mb.abc, mb.n_abc, rows_global, m, i, o, out)) != hipSuccess) return e;
	return hipSuccess;
}

} // namespace

namespace djbk {

size_t scene_tiles(long long m) { return (size_t)((m + (long long)TILE - 1) / (long long)TILE); }

hipError_t launch_scene_count_scan(hipStream_t s, const unsigned int *slots, int n_slots, long long m, const int32_t *material, const SceneScratch &sc)
{
	const unsigned int n_tiles = (unsigned int)scene_tiles(m);
	hipLaunchKernelGGL(k_scene_count, dim3((n_tiles + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, s, slots, (unsigned int)n_slots, (unsigned int)m,
	                   material, n_tiles, sc.tiles);
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_scene_scan, dim3(1), dim3(SCAN_BLOCK), 0, s, n_tiles, sc.tiles, sc.hdr);
	return hipGetLastError();
}

hipError_t launch_scene_eval(hipStream_t s, const SceneMembers &members, const unsigned int *slots, int n_slots, long long m, const int32_t *material,
                             const View &i, const View &o, const View &out, bool want_cos, const SceneScratch &scratch, bool merl_exact,
                             bool utia_exact, bool rows_global)
{
	if (m <= 0) return hipSuccess;
	if (m > SCENE_CHUNK_MAX) return hipErrorInvalidValue;
	return want_cos ? launch_all<2>(s, members, slots, n_slots, m, material, i, o, out, scratch, merl_exact, utia_exact, rows_global)
	                : launch_all<1>(s, members, slots, n_slots, m, material, i, o, out, scratch, merl_exact, utia_exact, rows_global);
}

} // namespace djbk
