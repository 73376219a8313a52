// djb_utia_hits.inc -- what every UTIA per-hit kernel shares (djb_kernels_utia_set.hip, djb_kernels_scene.hip, djb_kernels_scene_proxy.hip):
// the table's geometry and the Brdf of the exact path.  Included inside each file's anonymous namespace.
// The kernels stay written out.  Tier 1 (k_utia_set / k_scene_utia): on one body over a hit source (djb_hit_source.inc) k_utia_set did not
// keep its instructions (DESIGN.md 4.11.2).  Tier 2 (k_utia_set_fix / k_scene_utia_fix): they differ in what an inactive hit does (the
// set's tier 2 leaves tier 1's +0 alone unless it runs alone) and in where the indices of the "all" case come from.
#ifndef DJB_UTIA_MIN_WAVES
#define DJB_UTIA_MIN_WAVES 4
#endif
constexpr unsigned int TABLE_F4 = 288u * 288u * 8u;        // float4 per material
constexpr unsigned int NO_RECORD = 0xffffffffu;            // an inactive owner: its chunks are not requested
// tab = float4[M][663552]; the BYTE offset ((material * 663552 + 8 e + chunk) << 4) reaches 2.72e9 at DJB_UTIA_SET_MAX = 256 tables:
// beyond 2^31, below 2^32 -- formed and extended unsigned, the uniform base + 32-bit offset form of the LDS-direct load
static_assert(255ull * TABLE_F4 + 8ull * (288ull * 288ull - 1ull) + 7ull < (1ull << 28), "the byte offset of the last chunk fits 32 bits");

// the Brdf of the exact path (eval_one<KIND_UTIA>): kind utia, nothing else set; its `utia` becomes the hit's table per lane
inline Brdf utia_target()
{
	Brdf b;
	memset(&b, 0, sizeof b);
	b.kind = KIND_UTIA;
	return b;
}
