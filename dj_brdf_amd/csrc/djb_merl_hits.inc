// djb_merl_hits.inc -- the three per-hit MERL bodies, each written once over a hit source (djb_hit_source.inc): the set kernels of
// djb_kernels_merl_set.hip run them on a batch, the scene kernels of djb_kernels_scene.hip / djb_kernels_scene_proxy.hip on the list of
// the scene's MERL hits.  Included inside each file's anonymous namespace, after BLOCK and the source.  The kernels keep their
// __shared__ arrays and pass them in.  All three have the two-tier shape of k_merl_fast: tier 1 in place, the pairs it declines wait in a
// per-wave LDS queue (djb_worklist.hpp: recq_push / recq_drain) whose record carries the material id, one drain site finishes them with
// the exact index as dense waves; the trip count is workgroup-uniform and one extra trip flushes the queues.
constexpr long long MERL_TEXELS = 90LL * 90 * 180;

// material * 1458000 + index fits an int32 up to DJB_MERL_SET_MAX = 1024 tables, the BYTE offset (x 12) does not beyond table 245: the
// element index is formed in 64 bits
DJB_DEV v3 merl_set_texel(const MerlTexel *tex, unsigned int material, int idx)
{
	const MerlTexel t = tex[(unsigned long long)material * (unsigned long long)MERL_TEXELS + (unsigned long long)(unsigned int)idx];
	return mk(t.x, t.y, t.z);
}

// the part of a queue record all three bodies share: {k lo, k hi, material, i.xyz, o.xyz}
DJB_DEV void rec_pack(unsigned int *rec, long long k, unsigned int material, v3 i, v3 o)
{
	rec_put_k(rec, k); rec[2] = material; rec_put_v3(rec, 3, i); rec_put_v3(rec, 6, o);
}

// ---- eval (WANT 1) / evalp (WANT 2) per hit
template <int WANT, class S>
DJB_DEV void merl_eval_hits(const S &src, unsigned int (&s_q)[BLOCK / 64][9][RECQ_CAP], const MerlTexel *tex, View vi, View vo,
                            View vout, MerlGuard g, int merl_exact)
{
	typedef typename S::index index;
	if (src.none()) return;
	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	unsigned int (&q)[9][RECQ_CAP] = s_q[wave];
	unsigned int qn = 0;                                                           // wave-uniform
	const index cnt = src.count(), stride = src.stride();
	for (index j0 = src.start(); ; j0 += stride) {                                 // workgroup-uniform trip count; one extra trip flushes the queues
		const bool last = j0 >= cnt;
		bool amb = false;
		unsigned int id = 0u;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		index k = src.idle(j0, t);
		const unsigned int rem = last ? 0u : cnt - j0 >= (index)BLOCK ? (unsigned int)BLOCK : (unsigned int)(cnt - j0);
		if (t < rem) {
			k = src.at(j0, t);
			const bool act = src.id(k, id);
			const typename S::lane_t l = src.lane(j0, t, k);
			i = src.in3(vi, l); o = src.in3(vo, l);
			v3 fr = mk(0, 0, 0);                                                       // an inactive hit: +0, nothing read
			if (act) {
				int idx = 0;
				if (!merl_exact && merl_index_fast(i, o, g, idx)) {
					const v3 e = merl_set_texel(tex, id, idx);
					fr = (WANT & 2) ? scale(i.z, e) : e;                                   // brdf::evalp, dj_brdf.h:803-806
				} else amb = true;                                                      // the exact index finishes this pair
			}
			if (!amb) src.out3(vout, l, fr);
		}
		unsigned int rec[9];                                                       // built here, outside the branches above (djb_worklist.hpp)
		rec_pack(rec, (long long)k, id, i, o);
		recq_push(q, qn, lane, amb, rec);
		recq_drain(q, qn, lane, last, [&](const unsigned int *r) {
			const v3 iq = rec_v3(r, 3);
			const v3 e = merl_set_texel(tex, r[2], merl_index(iq, rec_v3(r, 6)));
			store3(vout, rec_k(r), (WANT & 2) ? scale(iq.z, e) : e);
		});
		if (last) break;
	}
}

// ---- the per-bounce step of dj_merl per hit: direction and pdf from a GGX or Beckmann lobe whose Params come per lane from the resident
// Params[M], the weight from table[material].  k_evalp_is_proxy<PKIND, KIND_MERL> with Params and the table base per lane
template <int PKIND, class S>
DJB_DEV void merl_is_hits(const S &src, double *s_glibc, unsigned long long *s_exp, unsigned int (&s_q)[BLOCK / 64][10][RECQ_CAP], Brdf pb,
                          const Params *params, const MerlTexel *tex, const float *u1a, const float *u2a, View vo, View vw_out,
                          View vi_out, float *out_pdf, MerlGuard g, int merl_exact)
{
	static_assert(PKIND == KIND_GGX || PKIND == KIND_BECKMANN, "the proxy of a MERL set is an analytic lobe");
	typedef typename S::index index;
	if (src.none()) return;                                                        // before the staging and its barrier
	GlibcTabs gt = glibc_tabs_global();
	if (PKIND == KIND_BECKMANN) {                                                  // logf / expf / powf of Beckmann's quantile functions
		gt = glibc_tabs_to_lds(s_glibc, threadIdx.x, BLOCK);
		const LdsTab e = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
		pb.exp_lds = e; gt.exp64 = e;
		__syncthreads();
	}
	pb.atan_lds = 0u;

	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	unsigned int (&q)[10][RECQ_CAP] = s_q[wave];
	unsigned int qn = 0;                                                           // wave-uniform
	const index cnt = src.count(), stride = src.stride();
	for (index j0 = src.start(); ; j0 += stride) {                                 // one extra trip flushes the queues
		const bool last = j0 >= cnt;
		bool amb = false;
		unsigned int id = 0u;
		v3 i_ = mk(0, 0, 0), o = mk(0, 0, 1); float pdf = 0.0f;                        // an inactive hit: +0 everywhere, nothing read
		index k = src.idle(j0, t);
		const unsigned int rem = last ? 0u : cnt - j0 >= (index)BLOCK ? (unsigned int)BLOCK : (unsigned int)(cnt - j0);
		if (t < rem) {
			k = src.at(j0, t);
			v3 w = mk(0, 0, 0);
			if (src.id(k, id)) {
				const typename S::lane_t l = src.lane(j0, t, k);
				const float u1 = src.in1(u1a, l), u2 = src.in1(u2a, l);
				o = src.in3(vo, l);
				const Params pp = params[id];
				// ---- proxy: direction, then the pdf-only arm of mf_eval_pdf on (i, o)
				i_ = mf_sample<PKIND>(pb, pp, u1, u2, o, gt);
				if (!(i_.z <= 0.0f)) {                                                  // the side check; a NaN i.z is evaluated
					v3 unused;
					mf_eval_pdf<PKIND, 4>(pb, pp, i_, o, unused, pdf);
					int idx = 0;
					if (!merl_exact && merl_index_fast(i_, o, g, idx))
						w = divs(scale(i_.z, merl_set_texel(tex, id, idx)), pdf);           // brdf::evalp = eval * i.z, dj_brdf.h:803-806
					else amb = true;                                                    // the exact index finishes this pair (below)
				}
			}
			const typename S::lane_t l = src.lane(j0, t, k);                           // again: the stores sit in another block than the loads
			src.out3(vi_out, l, i_); src.out1(out_pdf, l, pdf);
			if (!amb) src.out3(vw_out, l, w);
		}
		unsigned int rec[10];                                                      // built here, outside the branches above (djb_worklist.hpp)
		rec_pack(rec, (long long)k, id, i_, o); rec[9] = __float_as_uint(pdf);
		recq_push(q, qn, lane, amb, rec);
		recq_drain(q, qn, lane, last, [&](const unsigned int *r) {
			const v3 iq = rec_v3(r, 3);
			const v3 e = merl_set_texel(tex, r[2], merl_index(iq, rec_v3(r, 6)));
			store3(vw_out, rec_k(r), divs(scale(iq.z, e), __uint_as_float(r[9])));
		});
		if (last) break;
	}
}

// ---- the light sample (next-event estimation / MIS) per hit: for a GIVEN pair, evalp from table[material] and the proxy's pdf with
// params[material]; dj_merl::eval / ::pdf return 0 where cosTheta(wi) <= 0 || cosTheta(wo) <= 0 (a NaN z is evaluated): such a hit reads
// nothing and is never queued.  The pdf needs no table: it is stored at once and the record is the 9 words of merl_eval_hits.  The texel of
// a pair tier 1 decides is asked for BEFORE the pdf arithmetic and consumed after it.  Beckmann: the pdf arm calls exp alone -- its table
// is staged, the log / pow tables of mf_sample are not.
template <int PKIND, class S>
DJB_DEV void merl_light_hits(const S &src, unsigned long long *s_exp, unsigned int (&s_q)[BLOCK / 64][9][RECQ_CAP], Brdf pb, const Params *params,
                             const MerlTexel *tex, View vi, View vo, View vout, float *out_pdf, MerlGuard g,
                             int merl_exact)
{
	static_assert(PKIND == KIND_GGX || PKIND == KIND_BECKMANN, "the proxy of a MERL set is an analytic lobe");
	typedef typename S::index index;
	if (src.none()) return;
	if (PKIND == KIND_BECKMANN) {
		pb.exp_lds = glibc_exp_tab_to_lds(s_exp, threadIdx.x, BLOCK);
		__syncthreads();
	}
	pb.atan_lds = 0u;

	const unsigned int t = threadIdx.x, wave = t >> 6, lane = t & 63u;
	unsigned int (&q)[9][RECQ_CAP] = s_q[wave];
	unsigned int qn = 0;                                                           // wave-uniform
	const index cnt = src.count(), stride = src.stride();
	for (index j0 = src.start(); ; j0 += stride) {                                 // workgroup-uniform trip count; one extra trip flushes the queues
		const bool last = j0 >= cnt;
		bool amb = false;
		unsigned int id = 0u;
		v3 i = mk(0, 0, 1), o = mk(0, 0, 1);
		index k = src.idle(j0, t);
		const unsigned int rem = last ? 0u : cnt - j0 >= (index)BLOCK ? (unsigned int)BLOCK : (unsigned int)(cnt - j0);
		if (t < rem) {
			k = src.at(j0, t);
			const bool act = src.id(k, id);
			const typename S::lane_t l = src.lane(j0, t, k);
			i = src.in3(vi, l); o = src.in3(vo, l);
			v3 fr = mk(0, 0, 0); float pdf = 0.0f;                                     // inactive, or below the horizon: +0, nothing read
			if (act && !(i.z <= 0.0f || o.z <= 0.0f)) {                                // dj_merl.cpp:57-60, 69-72; a NaN z is evaluated
				const Params pp = params[id];                                           // asked for first: loads return in order, and the
				int idx = 0;                                                            // pdf must not wait for the texel behind them
				const bool decided = !merl_exact && merl_index_fast(i, o, g, idx);
				v3 e = mk(0, 0, 0);
				if (decided) e = merl_set_texel(tex, id, idx);                          // in flight across the pdf
				v3 unused;
				mf_eval_pdf<PKIND, 4>(pb, pp, i, o, unused, pdf);                       // microfacet::pdf, dj_brdf.h:1713-1730
				if (decided) fr = scale(i.z, e);                                        // brdf::evalp, dj_brdf.h:803-806
				else amb = true;                                                        // the exact index finishes this pair
			}
			src.out1(out_pdf, l, pdf);
			if (!amb) src.out3(vout, l, fr);
		}
		unsigned int rec[9];                                                       // built here, outside the branches above (djb_worklist.hpp)
		rec_pack(rec, (long long)k, id, i, o);
		recq_push(q, qn, lane, amb, rec);
		recq_drain(q, qn, lane, last, [&](const unsigned int *r) {
			const v3 iq = rec_v3(r, 3);
			const v3 e = merl_set_texel(tex, r[2], merl_index(iq, rec_v3(r, 6)));
			store3(vout, rec_k(r), scale(iq.z, e));
		});
		if (last) break;
	}
}
