// djb_internal.hpp -- launch interface between the C-ABI host code (djb_host.cpp) and the
// gfx950 kernels (djb_kernels_*.hip).  Not installed; the public surface is include/djb_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "djb_device.hpp"
#include "djb_microfacet_row.hpp"

namespace djbk {

using djbdev::Brdf;
using djbdev::Params;
using djbdev::View;

// workgroups of `block` threads for n units: one per `block` units, at most `cap` (the kernels stride over the batch beyond), at least one
inline int grid_capped(long long n, int block, long long cap)
{
	long long blocks = (n + block - 1) / block;
	if (blocks > cap) blocks = cap;
	if (blocks < 1) blocks = 1;
	return (int)blocks;
}

// dense batches address their arrays as uniform base + lane offset (load3_dense / store3_dense, djb_device_units.inc).  Two meanings:
// dense_strict -- the view is there and has stride 1; dense_or_null -- ... or the view is absent (an output the call does not ask for)
inline bool dense_strict(const View &v) { return v.stride == 1; }
inline bool dense_or_null(const View &v) { return v.stride == 1 || v.x == nullptr; }

// WANT bits: 1 eval, 2 evalp, 4 pdf (1 and 2 are exclusive)
hipError_t launch_eval(hipStream_t s, const Brdf &b, const Params &p, long long n,
                       const View &i, const View &o, const View &out_fr, float *out_pdf, int want);

// sample / evalp_is.  If u1 == nullptr the uniforms come from the on-chip counter RNG
// (seed_u1, seed_u2, start); out_w / out_pdf may be null-views (sample only).
// contract (DJB_OPT_CONTRACT_1E5): Beckmann and GGX `sample` may return directions within 1e-5 per component instead of the reference's bits
hipError_t launch_sample(hipStream_t s, const Brdf &b, const Params &p, long long n,
                         const float *u1, const float *u2, uint32_t seed_u1, uint32_t seed_u2,
                         unsigned long long start, const View &o, const View &out_i,
                         const View *out_w, float *out_pdf, bool contract = false);

// the Beckmann lobe's sample / evalp_is (djb_kernels_sample.hip: common path + deferred full path); launch_sample forwards here
hipError_t launch_sample_beckmann(hipStream_t s, const Brdf &b, const Params &p, long long n,
                                  const float *u1, const float *u2, uint32_t seed_u1, uint32_t seed_u2,
                                  unsigned long long start, const View &o, const View &out_i,
                                  const View *out_w, float *out_pdf, bool contract = false);
// ggx `sample` under DJB_OPT_CONTRACT_1E5: directions within 1e-5 per component (djb_kernels_sample.hip, ggx_sample_contract)
hipError_t launch_sample_ggx_contract(hipStream_t s, const Brdf &b, const Params &p, long long n, const float *u1, const float *u2,
                                      uint32_t seed_u1, uint32_t seed_u2, unsigned long long start, const View &o, const View &out_i);
bool sample_contract_supported(const Brdf &b, const Params &p);
// the contract-mode sampler against the full per-sample code on n generated samples (k_sample_ct_selftest)
hipError_t launch_sample_contract_selftest(hipStream_t s, const Brdf &b, const Params &p, long long n, uint32_t seed, unsigned long long start,
                                           int family, unsigned int *max_bits, unsigned long long *counters);
// directed search over the bit patterns of (u1, u2, o) for the largest contract-vs-exact difference (k_sample_ct_attack); u1, u2, o are updated in place
hipError_t launch_sample_contract_attack(hipStream_t s, const Brdf &b, const Params &p, long long n, float *u1, float *u2, const View &o, int iters,
                                         uint32_t seed, float *best, unsigned long long *counters);

// proxy importance sampling (djb_kernels_proxy.hip): i = proxy.sample(u1, u2, o), pdf = proxy.pdf(i, o), weight = target.evalp(i, o) / pdf,
// weight = 0 and pdf = 0 where i.z <= 0 -- one launch.  Targets: merl, utia, sgd, abc; proxies: ggx, beckmann, tabular, tabular_anisotropic
bool evalp_is_proxy_supported(int target_kind, int proxy_kind);
hipError_t launch_evalp_is_proxy(hipStream_t s, const Brdf &target, const Params &target_p, const Brdf &proxy, const Params &proxy_p, long long n,
                                 const float *u1, const float *u2, const View &o, const View &out_w, const View &out_i, float *out_pdf,
                                 bool merl_exact);
// the light sample of the same plugins (djb_kernels_proxy_light.hip): fr = target.evalp(i, o), pdf = proxy.pdf(i, o) of a GIVEN pair, both +0
// where i.z <= 0 || o.z <= 0 -- one launch, the pairs of kinds of evalp_is_proxy_supported
hipError_t launch_evalp_pdf_proxy(hipStream_t s, const Brdf &target, const Params &target_p, const Brdf &proxy, const Params &proxy_p, long long n,
                                  const View &i, const View &o, const View &out_fr, float *out_pdf, bool merl_exact);

// MERL material sets (djb_kernels_merl_set.hip): tex = MerlTexel[n_mat][1458000], material = n ids (outside [0, n_mat): an inactive hit,
// every output +0); eval / evalp per hit, and launch_evalp_is_proxy per hit with params[material] as the proxy's parameters.  One launch each;
// proxy: ggx or beckmann
hipError_t launch_merl_set_eval(hipStream_t s, const djbdev::MerlTexel *tex, int n_mat, long long n, const int32_t *material, const View &i,
                                const View &o, const View &out, bool want_cos, bool merl_exact);
hipError_t launch_merl_set_evalp_is_proxy(hipStream_t s, const Brdf &proxy, const Params *params, const djbdev::MerlTexel *tex, int n_mat, long long n,
                                          const int32_t *material, const float *u1, const float *u2, const View &o, const View &out_w,
                                          const View &out_i, float *out_pdf, bool merl_exact);
// the light sample per hit: evalp from table[material] and the proxy's pdf with params[material] of a GIVEN pair, both +0 where
// i.z <= 0 || o.z <= 0.  One launch
hipError_t launch_merl_set_evalp_pdf(hipStream_t s, const Brdf &proxy, const Params *params, const djbdev::MerlTexel *tex, int n_mat, long long n,
                                     const int32_t *material, const View &i, const View &o, const View &out_fr, float *out_pdf, bool merl_exact);

// per-pair params: rec = n x 5 floats; mode 0 = pdfparams records, mode 1 = LEAN texel moments composed with
// base5 = params_to_lrep(base) (unscaled), scale = dmapscale, lean_flags = DJB_LEAN_* as dj_beckmannconductor does;
// out_pp (optional, modes 1 and 2) receives the resolved pdfparams.  mode 2 = mode 1 with the record of pair k looked up in a
// resident LEAN map at (uv_k, lod_k): src is given, rec is not read
hipError_t launch_eval_pp(hipStream_t s, const Brdf &b, long long n, const View &i, const View &o,
                          const float *rec, int mode, const float *base5, float scale, int lean_flags, const View &out,
                          float *out_pdf, float *out_pp, int want, const djbdev::LeanSrc *src = nullptr);

// sample (out_w == NULL) / evalp_is with the same per-pair records
hipError_t launch_sample_pp(hipStream_t s, const Brdf &b, long long n, const float *u1, const float *u2, const View &o,
                            const float *rec, int mode, const float *base5, float scale, int lean_flags, const View &out_i,
                            const View *out_w, float *out_pdf, float *out_pp, const djbdev::LeanSrc *src = nullptr);

// LEAN maps (djb_leanmap.hip).  Images and texel blocks are device memory; texels: 2 float4 per texel, levels one after the other
hipError_t launch_dmap_to_nmap(hipStream_t s, int w, int h, const unsigned char *dmap, float scale, unsigned char *rgb);
hipError_t launch_leanmap_from_nmap(hipStream_t s, int w, int h, const unsigned char *rgb, int pixel_stride, float base_roughness, float4 *level0);
hipError_t launch_leanmap_from_moments(hipStream_t s, int w, int h, const float *moments5, int biased, float4 *level0);
hipError_t launch_leanmap_downsample(hipStream_t s, const float4 *src, int ws, int hs, float4 *dst, int wd, int hd);
hipError_t launch_leanmap_lookup(hipStream_t s, const djbdev::LeanSrc &src, long long n, float *out5);

// microfacet / radial queries; out.x holds scalar results (out.xyz for the Fresnel query)
hipError_t launch_query(hipStream_t s, const Brdf &b, const Params &p, int which, long long n,
                        const View &a, const View &bb, const View &c, const View &out);

hipError_t launch_io_to_hd(hipStream_t s, long long n, const View &i, const View &o,
                           const View &h, const View &d, bool inverse);
hipError_t launch_merl_index(hipStream_t s, long long n, const View &i, const View &o, int32_t *idx);
hipError_t launch_merl_keys(hipStream_t s, long long n, const View &i, const View &o, uint32_t *keys);     // tier-1 bin keys (djb_kernels_merl.hip)

// two-tier exact MERL lookup (djb_kernels_merl.hip): one kernel, the ambiguous pairs of tier 1 wait in per-wave LDS queues and are
// drained by the exact path as dense waves (no worklist in HBM, no second launch)
hipError_t launch_merl_twotier(hipStream_t s, const Brdf &b, long long n, const View &i, const View &o,
                               const View &out, float *out_pdf, int want);
hipError_t launch_merl_guard_stats(hipStream_t s, long long n, const View &i, const View &o,
                                   const float *guard6, unsigned int *max_bits, unsigned long long *counters);

// directed search for the worst |estimate - reference| / guard band: i / o are candidates in device memory, updated in place;
// best[n] receives each candidate's final ratio; counters = {evaluations, index mismatches among certain pairs, accepted moves}
hipError_t launch_merl_guard_attack(hipStream_t s, long long n, const View &i, const View &o, const float *guard6, int iters, uint32_t seed,
                                    float *best, unsigned long long *counters);

// MERL payload (3*n doubles) -> packed RGB texel table (pre-scaled, below-horizon zeroed); n = 1458000
hipError_t launch_merl_convert(hipStream_t s, const double *samples, long long n, djbdev::MerlTexel *table);
// UTIA payload (n = 3*288*288 doubles) -> float(max(0, s) * double(1.f/140.f)) in 288*288 records of 8 float4
hipError_t launch_utia_convert(hipStream_t s, const double *samples, long long n, float4 *table);

hipError_t launch_gen_directions(hipStream_t s, long long n, uint32_t seed, unsigned long long start,
                                 const View &out);
hipError_t launch_gen_uniforms(hipStream_t s, long long n, uint32_t seed, unsigned long long start,
                               float *out);
// utia eval / evalp (want 1, 2, 5, 6), two-tier: k_utia_v2 (no exact fall-backs; lists the undecided pairs) +
// k_eval_utia_fix for the pairs of the worklist (count: 16 bytes, list: cap entries).  contract: DJB_OPT_CONTRACT_1E5 -- the
// sRGB power of the decode on the fast transcendentals, everything else (cells, weights, the 16-tap sums) the reference's bits
hipError_t launch_utia_twotier(hipStream_t s, const Brdf &b, long long n, const View &i, const View &o, const View &out,
                               float *out_pdf, int want, unsigned int *list, unsigned int cap, unsigned int *count, bool contract);
// UTIA material sets (djb_kernels_utia_set.hip): tab = float4[n_mat][288 * 288 * 8], material = n ids (outside [0, n_mat): an inactive hit,
// +0); eval / evalp per hit with the two tiers of launch_utia_twotier (list / cap / count as there).  exact_only: the tier-2 kernel alone
// on every hit (reads a hit before it writes it; list and count are not used)
hipError_t launch_utia_set_eval(hipStream_t s, const float4 *tab, int n_mat, long long n, const int32_t *material, const View &i, const View &o,
                                const View &out, bool want_cos, unsigned int *list, unsigned int cap, unsigned int *count, bool exact_only);
// SGD / ABC model sets (djb_kernels_model_set.hip): rows = double[n_mat][model_set_row_stride(kind)] as create_model builds the single row
// (sgd: the 33 doubles + the fast tier's constants, abc: the 9 doubles), material = n ids (outside [0, n_mat): an inactive hit, +0); eval /
// evalp per hit, one launch.  rows_global: read the rows from global memory whatever n_mat is (DJB_OPT_MODEL_SET_ROWS_GLOBAL)
int model_set_row_stride(int kind);
hipError_t launch_model_set_eval(hipStream_t s, int kind, const double *rows, int n_mat, bool rows_global, long long n, const int32_t *material,
                                 const View &i, const View &o, const View &out, bool want_cos);
// ... and the two per-hit steps against the set's fitted tabular proxies (djb_kernels_model_set_proxy.hip).  tab: the resident proxy block,
// float[n_mat][3][res] (p22, sigma, qf of each material) followed by int n_qf[n_mat]; n_mat * res <= MODEL_SET_PROXY_MAX_ENTRIES keeps
// every byte offset into it below 2^31.  proxy_p: params::standard() as the single-material call resolves NULL proxy params.
// evalp_is_proxy: i = proxy_m.sample(u1, u2, o), pdf = proxy_m.pdf(i, o), weight = model_m.evalp(i, o) / pdf, weight = 0 and pdf = 0 where
// i.z <= 0; evalp_pdf: fr = model_m.evalp(i, o), pdf = proxy_m.pdf(i, o), both +0 where i.z <= 0 || o.z <= 0.  An inactive hit: +0 in every
// output.  One launch each; one trip of the grid covers MODEL_SET_PROXY_TRIP hits
constexpr long long MODEL_SET_PROXY_MAX_ENTRIES = 1LL << 27;
constexpr long long MODEL_SET_PROXY_TRIP = 256LL * 16 * 256;
struct ModelSetProxy { const float *tab; int res, shadow; };
hipError_t launch_model_set_evalp_is_proxy(hipStream_t s, int kind, const double *rows, int n_mat, bool rows_global, const ModelSetProxy &proxy,
                                           const Params &proxy_p, long long n, const int32_t *material, const float *u1, const float *u2,
                                           const View &o, const View &out_w, const View &out_i, float *out_pdf);
hipError_t launch_model_set_evalp_pdf(hipStream_t s, int kind, const double *rows, int n_mat, bool rows_global, const ModelSetProxy &proxy,
                                      const Params &proxy_p, long long n, const int32_t *material, const View &i, const View &o,
                                      const View &out_fr, float *out_pdf);
// Microfacet sets (djb_kernels_microfacet_set.hip): rows = MfRow[n_mat] (djb_microfacet_row.hpp) of ONE NDF kind, ggx or beckmann, material
// = n ids (outside [0, n_mat): an inactive hit, +0 in every output).  fr_kind: the Fresnel kind every row has, or -1 when they differ.
// eval: want bits as launch_eval_pp; sample: out_w == NULL gives sample(), else evalp_is().  One launch each.  rows_global: read the rows
// from global memory whatever n_mat is (DJB_OPT_MICROFACET_SET_ROWS_GLOBAL); by default up to microfacet_set_rows_lds() rows go to LDS,
// and the grid then has at most microfacet_set_grid_cap() workgroups
using djbdev::MfRow;
int microfacet_set_rows_lds();
long long microfacet_set_grid_cap();
hipError_t launch_microfacet_set_eval(hipStream_t s, int kind, const MfRow *rows, int n_mat, int fr_kind, bool rows_global, long long n,
                                      const int32_t *material, const View &i, const View &o, const View &out, float *out_pdf, int want);
hipError_t launch_microfacet_set_sample(hipStream_t s, int kind, const MfRow *rows, int n_mat, int fr_kind, bool rows_global, long long n,
                                        const int32_t *material, const float *u1, const float *u2, const View &o, const View &out_i, const View *out_w,
                                        float *out_pdf);
// Scenes (djb_kernels_scene.hip): hits on up to four member sets at once.  slots = n_slots words, kind (0 merl, 1 utia, 2 sgd, 3 abc; any
// other value: no material) << 16 | local id; a hit whose id is outside [0, n_slots) or whose slot has no material is inactive (+0).  One
// call partitions a chunk of m <= SCENE_CHUNK_MAX hits by kind on the device (three launches) and runs one kernel per member set that is
// there (utia: tier 1 + fix after a hipMemsetAsync of wl_count, or the fix kernel alone when utia_exact) on its segment of the index list.
// A null member is not launched.  Scratch, all device memory: hdr 8 words (count[4], offset[4]), tiles 4 * scene_tiles(m) words, list m
// words, wl_count 4 words, wl wl_cap words.
constexpr long long SCENE_CHUNK_MAX = 1LL << 26;
struct SceneMembers { const djbdev::MerlTexel *merl; int n_merl; const float4 *utia; int n_utia; const double *sgd; int n_sgd; const double *abc; int n_abc; };
struct SceneScratch { unsigned int *hdr, *tiles, *list, *wl_count, *wl; unsigned int wl_cap; };
size_t scene_tiles(long long m);
hipError_t launch_scene_eval(hipStream_t s, const SceneMembers &members, const unsigned int *slots, int n_slots, long long m, const int32_t *material,
                             const View &i, const View &o, const View &out, bool want_cos, const SceneScratch &scratch, bool merl_exact,
                             bool utia_exact, bool rows_global);
// the first two launches of a partition alone: tile counts, then their scan into positions, count[4] and offset[4] (scratch.tiles / .hdr)
hipError_t launch_scene_count_scan(hipStream_t s, const unsigned int *slots, int n_slots, long long m, const int32_t *material, const SceneScratch &scratch);
// ... and the two per-hit proxy steps on a scene (djb_kernels_scene_proxy.hip): the count and scan above, a scatter that stores the +0 of an
// inactive hit in every output of the call, then one kernel per member set on its segment of the list -- the body of the member set's proxy
// kernel (launch_merl_set_evalp_is_proxy / _evalp_pdf, launch_model_set_evalp_is_proxy / _evalp_pdf) and, for utia, of the single-material
// launch_evalp_is_proxy / launch_evalp_pdf_proxy with the hit's table and Params.  What they read beyond SceneMembers: the resident Params[M]
// of the merl and utia members and the proxy blocks of the model members (NULL where the scene has no such member).  proxy: the ggx or
// beckmann lobe of the merl and utia parts, not read without them; model_p: params::standard() for the fitted tabular proxies.
// scratch.wl / wl_count are not used: no kernel takes a second pass.  One trip of every per-kind grid covers SCENE_PROXY_TRIP hits
constexpr long long SCENE_PROXY_TRIP = 256LL * 16 * 256;
struct SceneProxies { const Params *merl, *utia; ModelSetProxy sgd, abc; };
hipError_t launch_scene_evalp_is_proxy(hipStream_t s, const SceneMembers &members, const SceneProxies &proxies, const Brdf *proxy, const Params &model_p,
                                       const unsigned int *slots, int n_slots, long long m, const int32_t *material, const float *u1, const float *u2,
                                       const View &o, const View &out_w, const View &out_i, float *out_pdf, const SceneScratch &scratch,
                                       bool merl_exact, bool rows_global);
hipError_t launch_scene_evalp_pdf_proxy(hipStream_t s, const SceneMembers &members, const SceneProxies &proxies, const Brdf *proxy, const Params &model_p,
                                        const unsigned int *slots, int n_slots, long long m, const int32_t *material, const View &i, const View &o,
                                        const View &out_fr, float *out_pdf, const SceneScratch &scratch, bool merl_exact, bool rows_global);
hipError_t launch_fast_trig_selftest(hipStream_t s, long long n, int mode, uint32_t first, uint32_t seed, unsigned long long *counters4);
// DJB_OPT_CONTRACT_1E5 (djb_kernels_contract.hip): GGX eval / evalp / pdf inside the 1e-5 value contract, two-tier like
// the MERL lookup, with a sharded worklist (list: cap records of 32 bytes in total, count: CONTRACT_SHARDS uint32, CONTRACT_COUNTER_STRIDE words apart: the record
// list is cut into that many equal segments).  Views must be dense (stride 1) and 16-byte aligned.
constexpr unsigned int WL_SHARDS = 64;
constexpr unsigned int WL_COUNTER_STRIDE = 32;         // words between two counters (one 128-byte line each)
constexpr unsigned int CONTRACT_SHARDS = WL_SHARDS, CONTRACT_COUNTER_STRIDE = WL_COUNTER_STRIDE;
constexpr float CT_RHO_MAX = 0.9f;
// launch-uniform constants of the contract-mode fast paths (filled by contract_params on the host, a kernel argument)
struct CtParams {
	float ax, ay, rho, s, rho_ay;      // microfacet::params (tx = ty = 0, mean normal = +z)
	float r_ax, r_t2;                  // float(1 / ax), float(1 / (ax ay s))
	float k_d;                         // float(r_t2 / pi): the constant factor of D
	float t2;                          // ax * ay * s as the reference rounds it (the divisor of mf_p22)
	double R_ax, R_t2;                 // 1 / ax and 1 / t2 to within 2^-52: fdiv_r's exact divisions (Beckmann)
	float f0[3], f1[3];                // schlick: f0 and 1 - f0
	float n2m1[3];                     // unpolarized: ior^2 - 1 per channel (ior >= CT_IOR_MIN)
	int shadow;
	// abc (model row kD[3] A[3] B C ior, dj_brdf.h:3608-3668)
	float kd_pi[3];                    // kD / pi as the reference rounds it: float(kD) * (1.0f / float(pi))
	float A[3], ior;
	double B, C;
	// sgd (model row rhoD rhoS alpha p f0 f1 kap lambda c k theta0, 3 doubles each; dj_brdf.h:3415-3500)
	float kd[3], ks[3], sf0[3], sf1[3], s1mf0[3];      // rhoD, rhoS, Fresnel f0, f1, 1 - f0 as floats (the reference's vec3::from_raw)
	double alpha[3], inv_alpha[3];
	float p_[3], lkap[3];                              // NDF exponent; log2(kap / pi)
	float lam[3], l2c[3], kk[3], th0_hi[3], th0_lo[3]; // g1: lambda, log2(c), k, theta0 = hi + lo
	float x_max[3], x_zero[3];                         // g1: tier-1 range of x = c t1^k (ct_params_sgd)
};
// false: brdf / params outside the fast path's domain
bool contract_params(const Brdf &b, const Params &p, const double *model_host, CtParams *c);
// model_host: the host copy of b.model (sgd / abc rows), or NULL
bool contract_supported(const Brdf &b, const Params &p, const double *model_host = nullptr);
hipError_t launch_eval_contract(hipStream_t s, const Brdf &b, const Params &p, const double *model_host, long long n, const View &i, const View &o,
                                const View &out, float *out_pdf, int want, unsigned int *list, unsigned int cap, unsigned int *count);
hipError_t launch_contract_selftest(hipStream_t s, const Brdf &b, const Params &p, const double *model_host, long long n, uint32_t seed_i, uint32_t seed_o,
                                    unsigned long long start, int family, unsigned int *max_bits, unsigned long long *counters);
hipError_t launch_guard_selftest(hipStream_t s, long long n, uint32_t seed, unsigned long long *counters);
hipError_t launch_model_fast_selftest(hipStream_t s, const Brdf &b, long long n, uint32_t seed, uint32_t first, unsigned long long *counters6);
hipError_t launch_libm_probe(hipStream_t s, int fn, long long n, const double *x, const double *y, double *out);
hipError_t launch_trig_sweep(hipStream_t s, int fn, uint32_t first, long long n, void *out);
hipError_t launch_histogram_xy(hipStream_t s, long long n, const View &v, int bins,
                               unsigned long long *counts);

// ---- the power-iteration fitter (djb::tabular ctor + fits), one workgroup per material
struct FitOut {           // device pointers, [n_mat][res] (fresnel [n_mat][res][3]); alphas [n_mat]
	float *p22, *sigma, *cdf, *qf, *fresnel;
	float *alpha_beckmann, *alpha_ggx;
	int *n_qf;            // number of valid qf entries per material (reference quirk, dj_brdf.h:2731)
};
// The two heavy passes of one material's fit -- the sigma quadrature (by rows) and the Fresnel-ratio pass (by
// (theta_d, theta_h) pairs) -- can be sliced over `parts` workgroups (fit_parts(n_mat)): parts - 1 helper
// workgroups per material redo the cheap phases before them and exchange their slices through sig_x [n_mat][res],
// the ratio scratch and the arrival counters sig_done [n_mat][2] (zeroed by launch_fit).
// fres_dirs (optional): one record of 5 floats per (theta_d, theta_h) pair of the Fresnel-ratio pass -- the outgoing direction (x = NaN
// for the pairs the reference skips) and the fitted lobe's two table coordinates that the pair's geometry fixes -- plus one trailing float
// (launch_fit_fresnel_dirs; fit_fresnel_dirs_floats(res) floats).  They depend on the resolution only, so the host computes them once per
// context and resolution instead of every workgroup of every fit recomputing 5 456 double rotations and 11 k fp64 libm calls; NULL:
// computed in place.
struct FitSplit { int parts; float *sig_x; unsigned int *sig_done; const float *fres_dirs; };
size_t fit_fresnel_dirs_floats(int res);
hipError_t launch_fit_fresnel_dirs(hipStream_t s, int res, const Params &std_p, float *recs);
int fit_parts(int n_mat, int n_cus);
// srcs: device array of n_mat Brdf views (all of kind `src_kind`); std_p: params::standard().
// km_scratch: n_mat*parts*(res-1)^2 doubles; ratio_scratch: n_mat*(res-1)*res*3 floats.
hipError_t launch_fit(hipStream_t s, const Brdf *srcs, int src_kind, const Params &std_p, int n_mat,
                      int res, int shadow, double *km_scratch, float *ratio_scratch,
                      const FitOut &out, const FitSplit &split);
size_t fit_lds_bytes(int res);
// query slots of a tabular(merl, res) fit and the MERL table index each one reads (-1: unused slot); idx: device, fit_merl_slots(res) ints
int fit_merl_slots(int res);
hipError_t launch_fit_merl_slots(hipStream_t s, int res, int32_t *idx);

// ---- tabular_anisotropic (djb_kernels_fit_aniso.hip): all pointers are device memory
struct AnisoScratch {
	int elev, azim;
	// outputs: grids are elev x azim, element (i_elev, j_azim) at [i + elev*j]
	float *p22, *sigma, *pdf1, *cdf1, *qf1, *pdf2, *cdf2, *qf2, *fres /* 3*elev */, *fit /* 10 */;
	int *counts;                               // [0] entries in qf1, [1] short qf2 rows, [2] entries in the reference's m_qf2
	// work arrays: N = (elev-1)*azim
	float *k1, *xo, *yo, *zo, *s1, *s2, *tn, *dn;   // N each
	double *v0, *v1;                                // N each
	float *terms;                                   // aniso_terms_count()
	float *ndf_tab;                                 // aniso_ndf_count()
	double *cosd;                                   // aniso_cosd_count(azim)
	float *sig_theta, *sig_sin; double *sig_cosd;   // aniso_sig_nodes() each
	float *ratio;                                   // 3*(elev-1)*elev
	float *probes;                                  // azim*8*(elev-1)
	float *rowk;                                    // azim
	float *qf2_rows; int *qf2_len;                  // elev*azim / azim: the rows of compute_qf2 before they are laid out
	int qf2_aligned;                                // 0: the reference's push_back layout; 1: every row at elev*k (DJB_OPT_ANISO_QF2_ALIGNED)
};
size_t aniso_terms_count();
size_t aniso_ndf_count();
size_t aniso_cosd_count(int azim);
size_t aniso_sig_nodes();
hipError_t launch_fit_aniso(hipStream_t s, const Brdf &src, const Params &std_p, const AnisoScratch &S, int shadow);

} // namespace djbk
