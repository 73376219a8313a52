// djb_cpu.hpp -- interface between the C ABI (djb_host.hip) and the product's HOST execution path
// (djb_cpu.cpp): the same per-unit code as the gfx950 kernels (djb_device.hpp), instantiated for the CPU with
// the host's own libm -- which is exactly what the reference (jdupuy/dj_brdf, a CPU library, dj_brdf.h:74-109)
// calls.  Two uses:
//   * a CPU context (djb_ctx_create(DJB_DEVICE_CPU)): every entry point of include/djb_hip.h on a machine
//     without a GPU -- BASELINE.json configs[0], "examples/merl_params.cpp ... CPU only, runs without a GPU";
//   * scalar-size DJB_MEM_HOST calls on a GPU context (the facade's one-pair virtuals, Mitsuba's per-hit calls):
//     n <= DJB_SCALAR_HOST_MAX units are evaluated here, on the caller's thread, with no staging, no launch and no
//     context mutex, from a host twin of the object's tables.
// Not a fallback for batches: a GPU context runs every batch above the scalar threshold on the GPU or fails.
// Nothing under oracle/ is used: that is test infrastructure.
#pragma once

#include <stdint.h>

#include "../../include/djb_hip.h"

// the host path's libm check (djb_cpu_libm.cpp): init() runs once, by the first context of either kind
namespace djbhostlibm {
extern int use_restated;
int init();
int atan_log_kat();
}

namespace djbcpu {

// handles: a CPU context / object starts with the same leading int as its GPU counterpart (djb_ctx: the device,
// djb_brdf: the device of the context that created it), which is how the C ABI tells them apart (device < 0).  The
// object carries its own copy: a handle may outlive its context (garbage collectors destroy them in any order).
inline bool is_cpu(const djb_ctx *c) { return c && *(const int *)c < 0; }
inline bool is_cpu(const djb_brdf *b) { return b && *(const int *)b < 0; }

// ---- context
djb_status ctx_create(djb_ctx **out);
djb_status ctx_destroy(djb_ctx *ctx);
djb_status timer_start(djb_ctx *ctx);
djb_status timer_stop_ms(djb_ctx *ctx, float *ms);
djb_ctx *twin_ctx();                 // process-wide CPU context that owns the host twins of GPU objects

// ---- constructors (same contracts as the djb_brdf_create_* entry points)
djb_status create_microfacet(djb_ctx *, int kind, const djb_fresnel_desc *, int shadow, djb_brdf **);
djb_status create_merl_from_memory(djb_ctx *, const double *samples, int64_t n, djb_brdf **);
djb_status create_merl_from_file(djb_ctx *, const char *path, djb_brdf **);
// a MERL object from an already converted texel table (n = 1458000 x 3 floats; copied)
djb_status create_merl_from_texels(djb_ctx *, const float *texels3, djb_brdf **);
djb_status create_utia_from_memory(djb_ctx *, const double *samples, djb_brdf **);
// a UTIA object from the converted table (288*288 records of 8 float4 = 32 floats; copied)
djb_status create_utia_from_records(djb_ctx *, const float *records, djb_brdf **);
djb_status create_utia_from_file(djb_ctx *, const char *path, djb_brdf **);
djb_status create_lambert(djb_ctx *, djb_brdf **);
djb_status create_model(djb_ctx *, int kind, const double *row, int count, djb_brdf **);
djb_status create_user_microfacet(djb_ctx *, const djb_user_ndf *, const djb_fresnel_desc *, int shadow, djb_brdf **);
djb_status create_tabular(djb_ctx *, const djb_brdf *src, int res, int shadow, djb_brdf **);
// a tabular / tabular_anisotropic object from tables fitted elsewhere (the host twin of a GPU-fitted object)
djb_status create_tabular_from_tables(djb_ctx *, int shadow, int res, const float *p22, const float *sigma, const float *cdf,
                                      const float *qf, int n_qf, const float *fresnel3, float alpha_b, float alpha_g, djb_brdf **);
djb_status create_aniso_from_tables(djb_ctx *, int shadow, int elev, int azim, const float *const tabs[8], const int counts[8],
                                    const float *fresnel3, const float fit10[10], int qf2_entries, djb_brdf **);
djb_status create_tabular_anisotropic(djb_ctx *, const djb_brdf *src, int elev, int azim, int shadow, djb_brdf **);
// fits of user-defined sources: the query slots of a fit (host code, any context) and the fit from per-slot samples
int fit_query_count(int res);
int fit_aniso_query_count(int elev, int azim);
djb_status fit_query_dirs(int res, float *i3, float *o3);
djb_status fit_aniso_query_dirs(int elev, int azim, float *i3, float *o3);
djb_status create_tabular_from_samples(djb_ctx *, int res, int shadow, const float *rgb, djb_brdf **);
djb_status create_tabular_anisotropic_from_samples(djb_ctx *, int elev, int azim, int shadow, const float *rgb, djb_brdf **);
djb_status destroy(djb_brdf *);
int kind(const djb_brdf *);
int get_shadow(const djb_brdf *);
djb_status set_shadow(djb_brdf *, int shadow);
djb_status set_fresnel(djb_brdf *, const djb_fresnel_desc *);
djb_status get_fresnel(const djb_brdf *, djb_fresnel_desc *out);
djb_status get_samples(const djb_brdf *, double *out, int64_t capacity, int64_t *count);
djb_status tabular_get(const djb_brdf *, int which, float *out, int *count);
djb_status tabular_fit(const djb_brdf *, float *alpha_beckmann, float *alpha_ggx);
djb_status aniso_get(const djb_brdf *, int which, float *out, int *count, int *elev, int *azim);
djb_status aniso_fit(const djb_brdf *, djb_params *beckmann, djb_params *ggx);

// ---- batch operators on host arrays (want bits: 1 eval, 2 evalp, 4 pdf)
djb_status eval(djb_ctx *, const djb_brdf *, int64_t n, const djb_vec3_view *i, const djb_vec3_view *o, const djb_params *,
                const djb_vec3_view *out_fr, float *out_pdf, int want);
// u1 == NULL: uniforms from the counter RNG (seed_u1, seed_u2, start); out_w == NULL: sample(), else evalp_is()
djb_status sample(djb_ctx *, const djb_brdf *, int64_t n, const float *u1, const float *u2, uint32_t seed_u1, uint32_t seed_u2,
                  uint64_t start, const djb_vec3_view *o, const djb_params *, const djb_vec3_view *out_w,
                  const djb_vec3_view *out_i, float *out_pdf);
// proxy importance sampling: i = proxy.sample, pdf = proxy.pdf(i, o), weight = target.evalp(i, o) / pdf; 0 and 0 where i.z <= 0.  Every pair of kinds
djb_status evalp_is_proxy(djb_ctx *, const djb_brdf *target, const djb_brdf *proxy, int64_t n, const float *u1, const float *u2,
                          const djb_vec3_view *o, const djb_params *target_params, const djb_params *proxy_params,
                          const djb_vec3_view *out_w, const djb_vec3_view *out_i, float *out_pdf);
// the light sample: fr = target.evalp(i, o), pdf = proxy.pdf(i, o) of a given pair; +0 and +0 where i.z <= 0 || o.z <= 0.  Every pair of kinds
djb_status evalp_pdf_proxy(djb_ctx *, const djb_brdf *target, const djb_brdf *proxy, int64_t n, const djb_vec3_view *i, const djb_vec3_view *o,
                           const djb_params *target_params, const djb_params *proxy_params, const djb_vec3_view *out_fr, float *out_pdf);
// MERL material sets on the host (include/djb_hip.h: djb_merl_set).  texels = MerlTexel[n_mat][1458000], params = djbdev::Params[n_mat]
// (both host memory, typed in djb_device.hpp); a hit whose id is outside [0, n_mat) gets +0 in every output.
// merl_set_member: the converted table of a dense MERL object of `ctx` (what djb_merl_set_create copies), or the reason it is refused
djb_status merl_set_member(const djb_ctx *ctx, const djb_brdf *b, int index, const void **texels);
// one plain djb_params resolved as the host path's single-material calls resolve it (-> one djbdev::Params)
djb_status merl_set_resolve_params(const djb_params *in, void *out_params);
djb_status merl_set_eval(djb_ctx *, const void *texels, int n_mat, int64_t n, const int32_t *material, const djb_vec3_view *i,
                         const djb_vec3_view *o, int want_cos, const djb_vec3_view *out_fr);
djb_status merl_set_evalp_is_proxy(djb_ctx *, const void *texels, const void *params, int n_mat, const djb_brdf *proxy, int64_t n,
                                   const int32_t *material, const float *u1, const float *u2, const djb_vec3_view *o,
                                   const djb_vec3_view *out_w, const djb_vec3_view *out_i, float *out_pdf);
djb_status merl_set_evalp_pdf(djb_ctx *, const void *texels, const void *params, int n_mat, const djb_brdf *proxy, int64_t n,
                              const int32_t *material, const djb_vec3_view *i, const djb_vec3_view *o, const djb_vec3_view *out_fr,
                              float *out_pdf);
// UTIA material sets on the host (include/djb_hip.h: djb_utia_set).  records = float4[n_mat][288 * 288 * 8] in host memory; a hit whose id
// is outside [0, n_mat) gets +0.  utia_set_member: the converted record table of a utia object of `ctx`, or the reason it is refused
djb_status utia_set_member(const djb_ctx *ctx, const djb_brdf *b, int index, const void **records);
djb_status utia_set_eval(djb_ctx *, const void *records, int n_mat, int64_t n, const int32_t *material, const djb_vec3_view *i,
                         const djb_vec3_view *o, int want_cos, const djb_vec3_view *out_fr);
// SGD / ABC model sets on the host (include/djb_hip.h: djb_model_set).  rows = double[n_mat][33 (sgd) or 9 (abc)] in host memory; a hit whose
// id is outside [0, n_mat) gets +0.  model_set_member: kind and row of an sgd / abc object of `ctx`, or the reason it is refused
djb_status model_set_member(const djb_ctx *ctx, const djb_brdf *b, int index, int *kind, const double **row);
djb_status model_set_eval(djb_ctx *, int kind, const double *rows, int n_mat, int64_t n, const int32_t *material, const djb_vec3_view *i,
                          const djb_vec3_view *o, int want_cos, const djb_vec3_view *out_fr);
// Microfacet sets on the host (include/djb_hip.h: djb_microfacet_set).  rows = djbdev::MfRow[n_mat] in host memory (djb_microfacet_row.hpp); a
// hit whose id is outside [0, n_mat) gets +0 in every output.  microfacet_set_member: kind, shadowing flag and Fresnel term (no spline
// points) of a ggx / beckmann object of `ctx`, or the reason it is refused.  eval: want bits 1 eval, 2 evalp, 4 pdf; sample: is = evalp_is()
djb_status microfacet_set_member(const djb_ctx *ctx, const djb_brdf *b, int index, int *kind, int *shadow, djb_fresnel_desc *fresnel);
djb_status microfacet_set_eval(djb_ctx *, int kind, const void *rows, int n_mat, int64_t n, const int32_t *material, const djb_vec3_view *i,
                               const djb_vec3_view *o, int want, const djb_vec3_view *out_fr, float *out_pdf);
djb_status microfacet_set_sample(djb_ctx *, int kind, const void *rows, int n_mat, int64_t n, const int32_t *material, const float *u1, const float *u2,
                                 const djb_vec3_view *o, bool is, const djb_vec3_view *out_w, const djb_vec3_view *out_i, float *out_pdf);
// Scenes on the host (include/djb_hip.h: djb_scene).  slots: n_slots packed words (djb_internal.hpp) in host memory; then the blocks of the
// members the scene has (NULL / 0 for the others, no slot names them) -- the MERL and UTIA tables with their resolved Params[M], the model
// rows with their fitted proxy blocks (model_set_fit_proxy below).  eval reads the tables and rows alone
struct SceneHost {
	const unsigned int *slots; int n_slots;
	const void *merl_texels, *merl_params, *utia_records, *utia_params;
	const double *sgd_rows; const float *sgd_block; int n_sgd, sgd_res, sgd_shadow;
	const double *abc_rows; const float *abc_block; int n_abc, abc_res, abc_shadow;
};
djb_status scene_eval(djb_ctx *, const SceneHost &, int64_t n, const int32_t *material, const djb_vec3_view *i, const djb_vec3_view *o, int want_cos,
                      const djb_vec3_view *out_fr);
// ... and the two per-hit proxy steps of a scene.  proxy: the ggx or beckmann lobe of the merl and utia parts, checked by the caller; NULL
// when the scene has neither
djb_status scene_evalp_is_proxy(djb_ctx *, const SceneHost &, const djb_brdf *proxy, int64_t n, const int32_t *material, const float *u1,
                                const float *u2, const djb_vec3_view *o, const djb_vec3_view *out_w, const djb_vec3_view *out_i, float *out_pdf);
djb_status scene_evalp_pdf(djb_ctx *, const SceneHost &, const djb_brdf *proxy, int64_t n, const int32_t *material, const djb_vec3_view *i,
                           const djb_vec3_view *o, const djb_vec3_view *out_fr, float *out_pdf);
// the set's fitted tabular proxies: block = float[n_mat][3][res] (p22, sigma, qf of tabular(model_m, res, shadow)) then int n_qf[n_mat], host
// memory; and the two per-hit steps against them (evalp_is_proxy / evalp_pdf_proxy above with target = model_m, proxy = that lobe, no params)
djb_status model_set_fit_proxy(djb_ctx *, int kind, const double *rows, int n_mat, int res, int shadow, float *block);
djb_status model_set_evalp_is_proxy(djb_ctx *, int kind, const double *rows, int n_mat, const float *block, int res, int shadow, int64_t n,
                                    const int32_t *material, const float *u1, const float *u2, const djb_vec3_view *o, const djb_vec3_view *out_w,
                                    const djb_vec3_view *out_i, float *out_pdf);
djb_status model_set_evalp_pdf(djb_ctx *, int kind, const double *rows, int n_mat, const float *block, int res, int shadow, int64_t n,
                               const int32_t *material, const djb_vec3_view *i, const djb_vec3_view *o, const djb_vec3_view *out_fr, float *out_pdf);
djb_status eval_pp(djb_ctx *, const djb_brdf *, int64_t n, const djb_vec3_view *i, const djb_vec3_view *o, const float *rec,
                   int mode, const float *base5, float scale, int lean_flags, int want, const djb_vec3_view *out_fr, float *out_pdf,
                   float *out_pp);
djb_status sample_pp(djb_ctx *, const djb_brdf *, int64_t n, const float *u1, const float *u2, const djb_vec3_view *o, const float *rec,
                     int mode, const float *base5, float scale, int lean_flags, const djb_vec3_view *out_w, const djb_vec3_view *out_i,
                     float *out_pdf, float *out_pp);
// LEAN maps in host memory (djb_leanmap.inc on the host): texels = 8 floats per texel, every level (djbdev::leanmap_total_texels)
void dmap_to_nmap(djb_ctx *, int w, int h, const unsigned char *dmap, float scale, unsigned char *rgb);
void leanmap_level0_from_nmap(djb_ctx *, int w, int h, const unsigned char *rgb, int pixel_stride, float base_roughness, float *texels);
void leanmap_level0_from_moments(djb_ctx *, int w, int h, const float *moments5, bool biased, float *texels);
void leanmap_build_pyramid(djb_ctx *, int lw, int lh, float *texels);
void leanmap_lookup(djb_ctx *, const float *texels, int lw, int lh, int64_t n, const float *uv, const float *lod, float *out5);
djb_status query(djb_ctx *, const djb_brdf *, int which, int64_t n, const djb_vec3_view *a, const djb_vec3_view *b,
                 const djb_vec3_view *c, const djb_params *, const djb_vec3_view *out);
djb_status io_hd(djb_ctx *, int64_t n, const djb_vec3_view *a, const djb_vec3_view *b, const djb_vec3_view *c,
                 const djb_vec3_view *d, bool inverse);
djb_status merl_index(djb_ctx *, int64_t n, const djb_vec3_view *i, const djb_vec3_view *o, int32_t *out);
djb_status fit_merl_batch(djb_ctx *, int n_mat, const double *const *tables, int res, int shadow, float *ab, float *ag,
                          float *p22, float *sigma, float *cdf, float *qf, float *fresnel);
djb_status fit_brdf_batch(djb_ctx *, int n_mat, const djb_brdf *const *srcs, int res, int shadow, float *ab, float *ag,
                          float *p22, float *sigma, float *cdf, float *qf, float *fresnel);
djb_status fit_merl_files(djb_ctx *, int n_files, const char *const *paths, int res, int shadow, int threads, float *ab,
                          float *ag, double *timing);
djb_status gen_directions(djb_ctx *, int64_t n, uint32_t seed, uint64_t start, const djb_vec3_view *out);
djb_status gen_uniforms(djb_ctx *, int64_t n, uint32_t seed, uint64_t start, float *out);
djb_status helper(int which, const float *in, float *out);    // djb_helper: the reference's file-static helpers, host arithmetic
djb_status histogram_xy(djb_ctx *, int64_t n, const djb_vec3_view *v, int bins, unsigned long long *counts);
// host values of trig site `host_fn` (djb_device.hpp TRIG_*; float sites < TRIG_DOUBLE, double sites from TRIG_DOUBLE)
// for the inputs with bit patterns first_bits .. first_bits + count - 1, compared with `dev` (a site evaluated on the
// GPU: floats or doubles); NaN == NaN.  Returns the number of differing inputs and stores the first `cap` of them
// (input bits, device bits, host bits; for a double site: input bits, |difference| in units of the last place, 0).
unsigned long long trig_sweep_compare(int host_fn, uint32_t first_bits, int64_t count, const void *dev, int threads,
                                      uint32_t *bad3, int cap);

} // namespace djbcpu

// helpers of djb_host.hip that the host path shares (scalar set-up code: microfacet::params resolution, the
// published sgd / abc rows, error reporting)
namespace djbk {
djb_status set_error(djb_status st, const char *fmt, ...);
djb_status resolve_device_params(const djb_params *in, float out9[9], int brdf_kind);   // Params {nx,ny,nz,ax,ay,rho,s,tx,ty}

// Does a resolved parameter set really follow this flagged djb_params (include/djb_hip.h: djb_params_cached)?  The flag is a promise
// about the bytes behind `c->p`, and a stray 0x100 in a plain djb_params must not turn into silently wrong parameters.  djb_params_resolve
// copies its inputs into the resolved form bit for bit (elliptic: a1, a2, phi_a; pdfparams: ax, ay, rho, tx_n, ty_n; standard: 1, 1, 0),
// so `r` carries a tag of `p`: it is held against `p`, and against what resolve can never write (NaN or negative ax / ay, |rho| > 1).
// No range test beyond that: rho == +-1 (elliptic(1, 1e-4, pi/4)) and every other set the plain path answers are legitimate.
static inline bool cached_params_follow(const djb_params_cached *c)
{
	const djb_params_resolved &r = c->r;
	if (!(r.ax >= 0.0f && r.ay >= 0.0f) || r.rho > 1.0f || r.rho < -1.0f) return false;
	auto same = [](float a, float b) { return __builtin_memcmp(&a, &b, sizeof a) == 0; };
	const float *v = c->p.v;
	switch (DJB_PARAMS_KIND(c->p.kind)) {
	case DJB_PARAMS_STANDARD: return r.a1 == 1.0f && r.a2 == 1.0f && same(r.phi_a, 0.0f) && same(r.tx_n, 0.0f) && same(r.ty_n, 0.0f);
	case DJB_PARAMS_ELLIPTIC: return same(r.a1, v[0]) && same(r.a2, v[1]) && same(r.phi_a, v[2]) && same(r.tx_n, 0.0f) && same(r.ty_n, 0.0f);
	case DJB_PARAMS_PDFPARAMS: return same(r.ax, v[0]) && same(r.ay, v[1]) && same(r.rho, v[2]) && same(r.tx_n, v[3]) && same(r.ty_n, v[4]);
	default: return false;
	}
}
} // namespace djbk
