// djb_scene_part.inc -- what the scene kernels of djb_kernels_scene.hip and djb_kernels_scene_proxy.hip share, included inside each file's
// anonymous namespace: the geometry of the partition, the slot table's decoding, the view of a partitioned batch, the list source of the per-kind kernels
// (the interface: djb_hit_source.inc) and the scatter kernel.
constexpr int BLOCK = 256;
constexpr unsigned int TILE = 512;                          // hits per wave of the partition kernels
constexpr unsigned int STEPS = TILE / 64u;
constexpr unsigned int K_MERL = 0, K_UTIA = 1, K_SGD = 2, K_ABC = 3, K_DEAD = 4;
constexpr unsigned int SLOT_NONE = 0xffffffffu;

// what every kernel reads of the batch: the slot table, the chunk's ids, and -- after the partition -- hdr = {count[4], offset[4]} and the list
struct Hits {
	const unsigned int *slots; unsigned int n_slots;
	const int32_t *mat;
	const unsigned int *hdr;
	const unsigned int *list;
};

// the slot of an id: nothing is read for an id outside [0, n_slots) (negative ids are >= 2^31 as unsigned)
DJB_DEV unsigned int slot_of(const unsigned int *slots, unsigned int n_slots, unsigned int raw) { return raw < n_slots ? slots[raw] : SLOT_NONE; }
DJB_DEV unsigned int kind_of(unsigned int slot) { const unsigned int q = slot >> 16; return q < 4u ? q : K_DEAD; }
// the local id of list entry k for the kernel of kind `q` with n_mat materials; false: not a hit of this kernel (the partition lists none)
DJB_DEV bool local_of(const Hits &h, unsigned int k, unsigned int q, unsigned int n_mat, unsigned int &local)
{
	const unsigned int slot = slot_of(h.slots, h.n_slots, (unsigned int)h.mat[k]);
	local = slot & 0xffffu;
	const bool ok = kind_of(slot) == q && local < n_mat;
	if (!ok) local = 0u;
	return ok;
}

// the tile of the calling wave in the partition kernels
DJB_DEV unsigned int wave_tile() { return (unsigned int)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6))); }

// ---- the list source: the hits of one kind behind the partition's list.  count and first are read once, here (uniform addresses: scalar
// loads; re-reading hdr[4 + kind] inside the loop cost instructions and SGPR spills).  Positions and hit indices are 32 bits wide
// (cnt <= 2^26, stride <= 2^20: j0 does not wrap); the streams are the plain load3 / store3 at k; an inactive hit has id 0.
struct ListHits {
	typedef unsigned int index;
	struct lane_t { unsigned int k; };
	Hits h; unsigned int kind, n_mat, cnt, first;
	DJB_DEV ListHits(const Hits &h_, unsigned int kind_, unsigned int n_mat_) : h(h_), kind(kind_), n_mat(n_mat_), cnt(h_.hdr[kind_]), first(h_.hdr[4 + kind_]) {}
	DJB_DEV bool none() const { return blockIdx.x * (unsigned int)BLOCK >= cnt; }      // the grid is sized for the chunk, an upper bound
	DJB_DEV index count() const { return cnt; }
	DJB_DEV index start() const { return blockIdx.x * (unsigned int)BLOCK; }
	DJB_DEV index stride() const { return gridDim.x * (unsigned int)BLOCK; }
	DJB_DEV index at(index j0, unsigned int t) const { return h.list[first + j0 + t]; }
	DJB_DEV index idle(index, unsigned int) const { return 0u; }
	DJB_DEV bool id(index k, unsigned int &id) const { return local_of(h, k, kind, n_mat, id); }
	DJB_DEV lane_t lane(index, unsigned int, index k, bool = false) const { const lane_t l = { k }; return l; }
	DJB_DEV v3 in3(const View &v, const lane_t &l) const { return load3(v, (long long)l.k); }
	DJB_DEV void out3(const View &v, const lane_t &l, v3 a) const { store3(v, (long long)l.k, a); }
	DJB_DEV float in1(const float *p, const lane_t &l) const { return p[l.k]; }
	DJB_DEV void out1(float *p, const lane_t &l, float x) const { p[l.k] = x; }
};

// ---- the partition's third step: every active hit writes its 32-bit index to its kind's segment of the list -- ballot + prefix popcount
// within the wave + the tile's offset: a stable counting sort, no atomic; a dead hit (id outside the table, a slot without material) gets
// dead(k) -- its +0 in every output of the call -- and is never read again
template <class DEAD>
DJB_DEV void scatter_hits(const unsigned int *slots, unsigned int n_slots, unsigned int m, const int32_t *mat, unsigned int n_tiles,
                          const unsigned int *tiles, unsigned int *list, DEAD dead)
{
	const unsigned int lane = threadIdx.x & 63u, tile = wave_tile();
	if (tile >= n_tiles) return;
	unsigned int off[4];                                                           // wave-uniform: where the tile's next hit of each kind goes
#pragma unroll
	for (unsigned int u = 0; u < 4u; ++u) off[u] = tiles[tile * 4u + u];
	const unsigned long long below = (1ull << lane) - 1ull;
	for (unsigned int s = 0; s < STEPS; ++s) {
		const unsigned int k = tile * TILE + s * 64u + lane;
		const bool live = k < m;
		unsigned int q = K_DEAD;
		if (live) q = kind_of(slot_of(slots, n_slots, (unsigned int)mat[k]));
#pragma unroll
		for (unsigned int u = 0; u < 4u; ++u) {
			const unsigned long long mask = __ballot(q == u);
			if (q == u) list[off[u] + (unsigned int)__popcll(mask & below)] = k;    // below count[u] + offset[u] <= m: the scan counted these hits
			off[u] += (unsigned int)__popcll(mask);
		}
		if (live && q == K_DEAD) dead(k);                                          // an inactive hit: +0, nothing read
	}
}
