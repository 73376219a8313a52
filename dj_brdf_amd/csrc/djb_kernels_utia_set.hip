// djb_kernels_utia_set.hip -- UTIA material sets: a batch of hits that lands on M resident UTIA record tables, eval / evalp per hit.
//
// The cells, angles, weights and tap order of a UTIA look-up depend on (i, o) alone (utia_cells_estimate / utia_record_index /
// utia_weights, djb_device_tables.inc), never on the material: a mixed batch computes them once per hit and only the base of the
// hit's two 128-byte records moves with its id.  No kind dispatch.  Two kernels, k_utia_v2 + k_eval_utia_fix (djb_kernels_utia.hip)
// with the table base per lane:
//   k_utia_set<WANT, DENSE>    tier 1, WANT 1 eval / 2 evalp: one hit per lane, the wave-cooperative record fetch straight into LDS, the
//                              reference's angles under it; lists the index of every active hit it does not decide
//   k_utia_set_fix<WANT>       tier 2: eval_one<KIND_UTIA> -- the reference as written -- on a Brdf whose `utia` is the hit's table, for
//                              the listed hits; for the whole batch if the list overflowed; alone (DJB_OPT_UTIA_EXACT_ONLY, in-place calls)
// A translation unit of its own: the code of k_utia_v2 does not move with this one.
// A hit whose id is outside [0, M) is inactive, as is a lane past the end of the batch: +0.0f in the three outputs, never listed, no
// address formed from its id, its chunks of the cooperative fetch not requested; a wave without an active lane skips fetch and
// arithmetic.  The per-unit functions are the ones k_utia_v2 calls, so an active hit has the bits of the single-material call.
// Addressing: tab = float4[M][663552]; the BYTE offset ((material * 663552 + 8 e + chunk) << 4) reaches 2.72e9 at DJB_UTIA_SET_MAX =
// 256 tables: beyond 2^31, below 2^32 -- formed and extended unsigned, the uniform base + 32-bit offset form of the LDS-direct load.
#include "djb_internal.hpp"
#include <string.h>

using namespace djbdev;

namespace {

constexpr int BLOCK = 256;
constexpr long long GRID_CAP = 256LL * 64;                 // as k_utia_v2

#include "djb_hit_source.inc"                              // BatchHits
#include "djb_utia_hits.inc"                               // DJB_UTIA_MIN_WAVES, TABLE_F4, NO_RECORD, utia_target

// 40 B per hit, touched once: non-temporal (k_utia_v2)
template <int WANT, bool DENSE>
__global__ __launch_bounds__(BLOCK, DJB_UTIA_MIN_WAVES) void k_utia_set(const float4 *tab, int n_mat, long long n, const int32_t *mat, View vi, View vo,
                                                                       View vout, unsigned int *list, unsigned int cap, unsigned int *count)
{
	__shared__ float4 s_tile[BLOCK / 64][384];
	__shared__ double s_atan[16];
	const lds_f64p T = atan_tab(atan_tab_to_lds(s_atan, threadIdx.x));
	__syncthreads();
	const long long stride = (long long)gridDim.x * BLOCK;
	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	typedef __attribute__((address_space(3))) void lds_void;
	typedef __attribute__((address_space(1))) const void glb_void;
	float4 *tile = s_tile[wave];
	for (long long k0 = (long long)blockIdx.x * BLOCK; k0 < n; k0 += stride) {     // k0: workgroup-uniform
		const long long k = k0 + t;
		const bool live = k < n;
		bool act = false;
		unsigned int id = 0u;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		if (live) {                                                                // 40 B per hit, touched once: non-temporal (k_utia_v2)
			const unsigned int raw = (unsigned int)__builtin_nontemporal_load(mat + k);
			i = DENSE ? load3_dense_nt(vi, k0, t) : load3(vi, k); o = DENSE ? load3_dense_nt(vo, k0, t) : load3(vo, k);
			act = raw < (unsigned int)n_mat;                                        // negative ids are >= 2^31 as unsigned
			id = act ? raw : 0u;
		}
		v3 fr = mk(0, 0, 0);                                                       // an inactive hit: +0
		bool ok = true;
		if (__ballot(act) != 0ull) {                                               // wave-uniform: a wave of dead hits fetches and computes nothing
			const UtiaCells c = utia_cells_estimate(i, o);
			int e[2];
			utia_record_index(c, e);                                                // clamped for any input: inside the material's table
			// first float4 of the hit's record a: at most 255 * 663552 + 8 * 82943 < 2^28
			unsigned int rec[2];
			rec[0] = act ? id * TABLE_F4 + 8u * (unsigned int)e[0] : NO_RECORD;
			rec[1] = act ? id * TABLE_F4 + 8u * (unsigned int)e[1] : NO_RECORD;
			float4 q[6];
			auto fetch = [&](int a) {
				unsigned int rec_src[6];                                                // the six shuffles first: one wait, not one per load
#pragma unroll
				for (unsigned int s = 0; s < 6u; ++s) {
					const unsigned int g = s * 64u + lane, r = (g * 10923u) >> 16;          // r = g / 6 for g < 384
					rec_src[s] = (unsigned int)__shfl((int)rec[a], (int)r);                 // record AND material from the owner
				}
#pragma unroll
				for (unsigned int s = 0; s < 6u; ++s) {
					const unsigned int g = s * 64u + lane, r = (g * 10923u) >> 16, chunk = g - 6u * r;
					if (rec_src[s] != NO_RECORD) {
						// uniform base + unsigned 32-bit byte offset (up to 2.72e9): the saddr form of the load, no 64-bit address arithmetic per lane
						const char *src = (const char *)tab + (size_t)((rec_src[s] + chunk) << 4);
						__builtin_amdgcn_global_load_lds((glb_void *)src, (lds_void *)(tile + s * 64u), 16, 0, 0);
					}
				}
			};
			auto take = [&]() {
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                        // this wave's LDS-direct loads have landed
#pragma unroll
				for (unsigned int j = 0; j < 6u; ++j) q[j] = tile[lane * 6u + j];
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
			if (DENSE) store3_dense_nt(vout, k0, t, fr); else store3(vout, k, fr);
			if (__builtin_expect(act & !ok, 0)) {
				const unsigned int slot = atomicAdd(count, 1u);
				if (slot < cap) list[slot] = (unsigned int)k;
			}
		}
	}
}

// alone: no tier 1 ran -- every hit of the batch, inactive ones stored as +0, `count` not read; a hit is read before it is written
template <int WANT>
__global__ __launch_bounds__(BLOCK) void k_utia_set_fix(Brdf b, const float4 *tab, int n_mat, long long n, const int32_t *mat, View vi, View vo, View vout,
                                                        const unsigned int *list, unsigned int cap, const unsigned int *count, int alone)
{
	const unsigned int c = alone ? 0u : *count;
	const bool all = alone || c > cap;                           // overflow: redo the whole batch
	const long long m = all ? n : (long long)c;
	const Params none = {};
	const long long stride = (long long)gridDim.x * BLOCK;
	for (long long j = (long long)blockIdx.x * BLOCK + threadIdx.x; j < m; j += stride) {
		const long long k = all ? j : (long long)list[j];
		const unsigned int id = (unsigned int)mat[k];
		v3 fr = mk(0, 0, 0); float pdf = 0.0f;
		if (id < (unsigned int)n_mat) {
			b.utia = tab + (size_t)id * (size_t)TABLE_F4;
			eval_one<KIND_UTIA, WANT>(b, none, load3(vi, k), load3(vo, k), fr, pdf);
		} else if (!alone) continue;                              // an inactive hit keeps tier 1's +0
		store3(vout, k, fr);
	}
}

template <int WANT>
hipError_t launch_set(hipStream_t s, const float4 *tab, int n_mat, long long n, const int32_t *mat, const View &i, const View &o, const View &out,
                      unsigned int *list, unsigned int cap, unsigned int *count, bool exact_only)
{
	const Brdf b = utia_target();
	dim3 t(BLOCK);
	if (exact_only) {
		hipLaunchKernelGGL((k_utia_set_fix<WANT>), dim3(djbk::grid_capped(n, BLOCK, GRID_CAP)), t, 0, s, b, tab, n_mat, n, mat, i, o, out, nullptr, 0u, nullptr, 1);
		return hipGetLastError();
	}
	hipError_t e = hipMemsetAsync(count, 0, 16, s);
	if (e != hipSuccess) return e;
	dim3 g(djbk::grid_capped(n, BLOCK, GRID_CAP));
	if (djbk::dense_strict(i) && djbk::dense_strict(o) && djbk::dense_strict(out))
		hipLaunchKernelGGL((k_utia_set<WANT, true>), g, t, 0, s, tab, n_mat, n, mat, i, o, out, list, cap, count);
	else
		hipLaunchKernelGGL((k_utia_set<WANT, false>), g, t, 0, s, tab, n_mat, n, mat, i, o, out, list, cap, count);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL((k_utia_set_fix<WANT>), dim3(64), t, 0, s, b, tab, n_mat, n, mat, i, o, out, list, cap, count, 0);
	return hipGetLastError();
}

} // namespace

namespace djbk {

hipError_t launch_utia_set_eval(hipStream_t s, const float4 *tab, int n_mat, long long n, const int32_t *material, const View &i, const View &o,
                                const View &out, bool want_cos, unsigned int *list, unsigned int cap, unsigned int *count, bool exact_only)
{
	if (n <= 0) return hipSuccess;
	return want_cos ? launch_set<2>(s, tab, n_mat, n, material, i, o, out, list, cap, count, exact_only)
	                : launch_set<1>(s, tab, n_mat, n, material, i, o, out, list, cap, count, exact_only);
}

} // namespace djbk
