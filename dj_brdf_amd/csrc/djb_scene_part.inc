// djb_scene_part.inc -- what the scene kernels of djb_kernels_scene.hip and djb_kernels_scene_proxy.hip share, included inside each file's
// anonymous namespace: the geometry of the partition, the slot table's decoding, the view of a partitioned batch, and the MERL record.
constexpr int BLOCK = 256;
constexpr unsigned int TILE = 512;                          // hits per wave of the partition kernels
constexpr unsigned int STEPS = TILE / 64u;
constexpr unsigned int K_MERL = 0, K_UTIA = 1, K_SGD = 2, K_ABC = 3, K_DEAD = 4;
constexpr unsigned int SLOT_NONE = 0xffffffffu;
constexpr long long MERL_TEXELS = 90LL * 90 * 180;
constexpr unsigned int TABLE_F4 = 288u * 288u * 8u;         // float4 per utia material

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

// ---- merl: the texel of a material and the part of a queue record every MERL kernel shares, {k lo, k hi, material, i.xyz, o.xyz}
DJB_DEV v3 merl_set_texel(const MerlTexel *tex, unsigned int material, int idx)
{
	const MerlTexel t = tex[(unsigned long long)material * (unsigned long long)MERL_TEXELS + (unsigned long long)(unsigned int)idx];
	return mk(t.x, t.y, t.z);
}
DJB_DEV void rec_pack(unsigned int *rec, long long k, unsigned int material, v3 i, v3 o)
{
	rec_put_k(rec, k); rec[2] = material; rec_put_v3(rec, 3, i); rec_put_v3(rec, 6, o);
}
