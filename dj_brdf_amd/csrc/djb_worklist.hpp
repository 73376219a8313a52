// djb_worklist.hpp -- device helpers shared by the two-tier kernels:
//   * 16-byte non-temporal stream accesses and the per-wave LDS staging of the global tier-2 worklist (wl_push / wl_flush:
//     djb_kernels_merl.hip, djb_kernels_contract.hip);
//   * the extra-trip record queue (recq_push / recq_drain and the record codec): the per-wave LDS queue of the pairs MERL's tier 1
//     declines in k_evalp_pdf_proxy, k_merl_set_fast, k_evalp_is_proxy_merl_set and k_merl_set_evalp_pdf (k_evalp_is_proxy follows the
//     same protocol with the code written out: through the helper it took 2 more VGPRs, see djb_kernels_proxy.hip);
//   * stage_table: the LDS table-staging step of k_eval, k_sample, k_evalp_is_proxy and k_evalp_pdf_proxy.
// NOT served by the record queue, on purpose: merl_queue / merl_drain (djb_kernels_merl.hip) and the queues of k_eval_bk_sharp and
// k_sample_bk.  Theirs is another protocol -- a trailing drain instead of an extra trip, float4 placeholder stores that must be waited
// for before the drain's stores, four pushes per iteration into 320 slots, a 32-bit k -- and routing merl_queue through recq_push
// moved the code of k_merl_fast_v4, the benchmark's default kernel (+1 / +4 instructions).  They stay as they are.
#pragma once
#include "djb_device.hpp"

namespace djbdev {

constexpr unsigned int WBUF = 128;   // per-wave LDS staging slots for worklist records (7 dwords each)

// 16-byte accesses for the streams that are touched exactly once.  DJB_STREAM_LOAD_POLICY / DJB_STREAM_STORE_POLICY pick
// the cache-policy bits (0 = nt through the compiler's builtin; 1 = sc1, 2 = sc0 sc1, 3 = sc0 sc1 nt, 4 = plain: inline asm):
// what the streams leave behind in the XCD's L2 decides how much of it the table gathers keep (profiles/r04/merl_stream_policy.txt)
#ifndef DJB_STREAM_LOAD_POLICY
#define DJB_STREAM_LOAD_POLICY 0
#endif
#ifndef DJB_STREAM_STORE_POLICY
#define DJB_STREAM_STORE_POLICY 0
#endif
typedef float nt_v4f __attribute__((ext_vector_type(4)));
#if DJB_STREAM_LOAD_POLICY == 0
DJB_DEV float4 nt_load4(const float4 *p)
{
	nt_v4f v = __builtin_nontemporal_load((const nt_v4f *)p);
	return make_float4(v.x, v.y, v.z, v.w);
}
DJB_DEV void nt_load_wait6(float4 &, float4 &, float4 &, float4 &, float4 &, float4 &) {}
#else
DJB_DEV float4 nt_load4(const float4 *p)
{
	nt_v4f v;
#if DJB_STREAM_LOAD_POLICY == 1
	asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory");
#elif DJB_STREAM_LOAD_POLICY == 2
	asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v) : "v"(p) : "memory");
#elif DJB_STREAM_LOAD_POLICY == 3
	asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1 nt" : "=v"(v) : "v"(p) : "memory");
#else
	asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
#endif
	return make_float4(v.x, v.y, v.z, v.w);
}
// the compiler does not count loads issued from inline asm: wait for them here, with the six results as operands so
// that no use can be scheduled ahead of the wait
DJB_DEV void nt_load_wait6(float4 &a, float4 &b, float4 &c, float4 &d, float4 &e, float4 &f)
{
	asm volatile("s_waitcnt vmcnt(0)" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w),
	             "+v"(c.x), "+v"(c.y), "+v"(c.z), "+v"(c.w) :: "memory");
	asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z), "+v"(d.w), "+v"(e.x), "+v"(e.y), "+v"(e.z), "+v"(e.w),
	             "+v"(f.x), "+v"(f.y), "+v"(f.z), "+v"(f.w) :: "memory");
}
#endif
DJB_DEV void nt_store4(float a, float b, float c, float d, float4 *p)
{
	nt_v4f v = { a, b, c, d };
#if DJB_STREAM_STORE_POLICY == 0
	__builtin_nontemporal_store(v, (nt_v4f *)p);
#elif DJB_STREAM_STORE_POLICY == 1
	asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
#elif DJB_STREAM_STORE_POLICY == 2
	asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
#elif DJB_STREAM_STORE_POLICY == 3
	asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
#else
	asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
#endif
}

// ---- per-wave worklist staging.  Ambiguous pairs are staged per wave in LDS (no barrier needed: one
// wave, in-order LDS) and flushed with ONE global atomic per flush: a returning atomic per ambiguous
// lane (~8e6 per 1e9 pairs on one address) costs more than the whole kernel.  A record is
// {k, i.xyz, o.xyz, pad} = two uint4, so the fix-up kernel streams its inputs instead of gathering them.
typedef unsigned int WaveBuf[7][WBUF];

DJB_DEV void wl_flush(WaveBuf &wb, unsigned int &wcount, int lane, uint4 *list, unsigned int cap,
                      unsigned int *count)
{
	unsigned int base = 0;
	if (lane == 0) base = atomicAdd(count, wcount);
	base = __shfl(base, 0);
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	for (unsigned int j = lane; j < wcount; j += 64)
		if (base + j < cap) {                                    // beyond cap: fix-up kernel rescans
			list[2 * (size_t)(base + j)] = make_uint4(wb[0][j], wb[1][j], wb[2][j], wb[3][j]);
			list[2 * (size_t)(base + j) + 1] = make_uint4(wb[4][j], wb[5][j], wb[6][j], 0u);
		}
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	wcount = 0;
}

DJB_DEV void wl_push(WaveBuf &wb, unsigned int &wcount, int lane, uint4 *list, unsigned int cap,
                     unsigned int *count, bool amb, unsigned int k, v3 i, v3 o)
{
	unsigned long long mask = __ballot(amb);
	if (!mask) return;
	unsigned int c = (unsigned int)__popcll(mask);
	if (wcount + c > WBUF) wl_flush(wb, wcount, lane, list, cap, count);
	if (amb) {
		unsigned int slot = wcount + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
		wb[0][slot] = k;
		wb[1][slot] = __float_as_uint(i.x); wb[2][slot] = __float_as_uint(i.y); wb[3][slot] = __float_as_uint(i.z);
		wb[4][slot] = __float_as_uint(o.x); wb[5][slot] = __float_as_uint(o.y); wb[6][slot] = __float_as_uint(o.z);
	}
	wcount += c;
}

// ---- the extra-trip record queue: the per-wave LDS queue of the pairs tier 1 declines, W words per record.  The kernel's batch loop
// makes one extra trip (`last`) that only flushes.  Capacity: fewer than 64 wait when an iteration starts and an iteration adds at
// most 64 (one unit per lane).  One wave, in-order LDS: no barrier, no atomics.
// The record is packed OUTSIDE the tier-1 branches, from values that live across them, as merl_queue's callers pass k, i, o: packed
// inside the declining branch, the k word of a pair tier 1 declined came out as 0 in the generated code (the fp64-only path kept it).
constexpr unsigned int RECQ_CAP = 128;
template <int W, unsigned int CAP>
DJB_DEV void recq_push(unsigned int (&q)[W][CAP], unsigned int &qn, unsigned int lane, bool amb, const unsigned int (&rec)[W])
{
	const unsigned long long mask = __ballot(amb);
	if (!mask) return;
	if (amb) {
		const unsigned int j = qn + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
		for (int w = 0; w < W; ++w) q[w][j] = rec[w];
	}
	qn += (unsigned int)__popcll(mask);
}
// while a full wave of records waits -- or, on the last trip, any -- hand `finish` one record per lane
template <int W, unsigned int CAP, class Finish>
DJB_DEV void recq_drain(unsigned int (&q)[W][CAP], unsigned int &qn, unsigned int lane, bool last, Finish finish)
{
	while (qn >= 64u || (last && qn)) {
		const unsigned int cnt = qn < 64u ? qn : 64u;
		qn -= cnt;
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		if (lane < cnt) {
			unsigned int rec[W];
#pragma unroll
			for (int w = 0; w < W; ++w) rec[w] = q[w][qn + lane];
			finish(rec);
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
	}
}
// the record codec: the 64-bit unit index k in words 0-1, a v3 at any word index; the caller owns the word order
DJB_DEV void rec_put_k(unsigned int *rec, long long k)
{
	rec[0] = (unsigned int)((unsigned long long)k & 0xffffffffull); rec[1] = (unsigned int)((unsigned long long)k >> 32);
}
DJB_DEV long long rec_k(const unsigned int *rec) { return (long long)(((unsigned long long)rec[1] << 32) | rec[0]); }
DJB_DEV void rec_put_v3(unsigned int *rec, int w, v3 a) { rec[w] = __float_as_uint(a.x); rec[w + 1] = __float_as_uint(a.y); rec[w + 2] = __float_as_uint(a.z); }
DJB_DEV v3 rec_v3(const unsigned int *rec, int w) { return mk(__uint_as_float(rec[w]), __uint_as_float(rec[w + 1]), __uint_as_float(rec[w + 2])); }

// ---- a table into the workgroup's LDS staging area `tab` (TAB_LDS floats, `used` of them taken): a null, empty or too large table
// stays in global memory; otherwise it is copied by the BS threads, `src` is redirected and `used` advances.  What a kernel stages, in
// which order, its budget and the barrier after the last table stay with the kernel.
template <int BS, int TAB_LDS>
DJB_DEV void stage_table(float (&tab)[TAB_LDS], int &used, const float *&src, int count)
{
	if (src == nullptr || count <= 0 || used + count > TAB_LDS) return;
	float *dst = tab + used;
	for (int k = threadIdx.x; k < count; k += BS) dst[k] = src[k];
	src = dst; used += count;
}

} // namespace djbdev
