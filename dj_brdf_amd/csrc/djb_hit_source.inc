// djb_hit_source.inc -- where a lane of a per-hit kernel gets its hit.  The bodies of the set and scene kernels (djb_merl_hits.inc,
// djb_model_hits.inc) are written once over a hit SOURCE; this is the batch source of the set calls.  The list source
// of the scene calls is ListHits (djb_scene_part.inc).  Included inside each file's anonymous namespace, after BLOCK.
//
// Two shapes.  The queue bodies (MERL) hold their loop: its exit is a break at the bottom.  The one-hit-per-lane bodies (sgd / abc eval and
// sampling) are written per TRIP and the kernel holds the loop
//     const S src(...); if (src.none()) return; <stage>; const index stride = src.stride();
//     for (index j0 = src.start(); j0 < src.count(); j0 += stride) <kind>_trip(src, j0, ...);
// because a `for` with its test at the top, inlined from a function, leaves the kernel's return AFTER the loop's blocks where the
// written-out kernel has it before them, and instruction selection then emits the latch compare with the other polarity.
// What a body asks of a source S (trips are BLOCK positions wide, j0 is workgroup-uniform):
//   S::index                       the type of a position and of a hit index k
//   none()                         this workgroup has no position at all: the body leaves before it stages anything
//   count(), start(), stride()     the positions, the workgroup's first one, the grid's step
//   at(j0, t), idle(j0, t)         the hit index of lane t in trip j0; the value k has in a lane outside the trip (it reaches the queue record)
//   id(k, id)                      the material id of hit k, and whether the hit is active
//   lane(j0, t, k[, dense_only])   the lane's handle for one block of accesses (taken again where the stores sit in another block;
//                                  dense_only: a block whose strided form did not take the offset)
//   in3 / in1 / out3 / out1        a v3 / scalar stream at the handle
//
// BatchHits<DENSE, OFF, NT>: position = hit index, 64 bits; the id stream is non-temporal and an inactive hit keeps its RAW id.
//   DENSE  every view has stride 1: uniform base + the lane's 32-bit offset; else the strided load3 / store3 at k
//   OFF    the lane's offset goes through lane_byte_offset() once per handle (dense_off); else dense_at(t)
//   NT     non-temporal streams (the scalar streams also where strided)
// Which kernel takes which was decided from register counts (djb_device_units.inc, the kernels' files): the choices are kept per kernel.
template <bool DENSE, bool OFF, bool NT>
struct BatchHits {
	typedef long long index;
	struct lane_t { long long j0; unsigned int a; long long k; };
	long long n; const int32_t *mat; unsigned int n_mat;
	DJB_DEV BatchHits(long long n_, const int32_t *mat_, int n_mat_) : n(n_), mat(mat_), n_mat((unsigned int)n_mat_) {}
	DJB_DEV bool none() const { return false; }
	DJB_DEV index count() const { return n; }
	DJB_DEV index start() const { return (long long)blockIdx.x * BLOCK; }
	DJB_DEV index stride() const { return (long long)gridDim.x * BLOCK; }
	DJB_DEV index at(index j0, unsigned int t) const { return j0 + t; }
	DJB_DEV index idle(index j0, unsigned int t) const { return j0 + t; }
	DJB_DEV bool id(index k, unsigned int &id) const
	{
		id = (unsigned int)__builtin_nontemporal_load(mat + k);
		return id < n_mat;                                                         // negative ids are >= 2^31 as unsigned
	}
	DJB_DEV lane_t lane(index j0, unsigned int t, index k, bool dense_only = false) const
	{
		const lane_t l = { j0, OFF && (DENSE || !dense_only) ? lane_byte_offset(t) : t, k };
		return l;
	}
	DJB_DEV v3 in3(const View &v, const lane_t &l) const
	{
		if (!DENSE) return load3(v, l.k);
		return !OFF ? load3_dense_nt(v, l.j0, l.a) : NT ? load3_dense_off_nt(v, l.j0, l.a) : load3_dense_off(v, l.j0, l.a);
	}
	DJB_DEV void out3(const View &v, const lane_t &l, v3 a) const
	{
		if (!DENSE) store3(v, l.k, a);
		else if (!OFF) store3_dense_nt(v, l.j0, l.a, a);
		else if (NT) store3_dense_off_nt(v, l.j0, l.a, a);
		else store3_dense_off(v, l.j0, l.a, a);
	}
	DJB_DEV float in1(const float *p, const lane_t &l) const
	{
		const float *q = !DENSE ? p + l.k : OFF ? dense_off(p + l.j0, l.a) : dense_at(p + l.j0, l.a);
		return NT ? __builtin_nontemporal_load(q) : *q;
	}
	DJB_DEV void out1(float *p, const lane_t &l, float x) const
	{
		float *q = !DENSE ? p + l.k : OFF ? dense_off(p + l.j0, l.a) : dense_at(p + l.j0, l.a);
		if (NT) __builtin_nontemporal_store(x, q); else *q = x;
	}
};
