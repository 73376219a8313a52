// scene_proxy_facade.cpp -- the two per-hit proxy steps of djb::scene and the proxy parameters of djb::utia_set in the djb:: facade
// (include/djb_hip.hpp): a scene over a utia set of two synthetic tables (parameters isotropic(0.3) and elliptic(0.2, 0.4, 0.3)) and an sgd
// model set of two published rows with its fitted proxies (resolution 24), slots {utia 0, sgd 1, none, utia 1, sgd 0}; evalp_is_proxy and
// evalp_pdf_proxy of a batch of hits (ids outside the table and on the slot without material included) held, bit for bit, against
// djb::utia::evalp_is_proxy / evalp_pdf_proxy with the material's parameters and djb::model_set::evalp_is_proxy / evalp_pdf_proxy.
// tests/test_scene_proxy_host.py runs it on the CPU context (DJB_DEVICE=cpu).  Prints "<n> hits checked, <d> differ"; exit 1 if d != 0.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "dj_brdf.h"

static unsigned int bits(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }
static bool same(const djb::vec3 &a, const djb::vec3 &b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y) && bits(a.z) == bits(b.z); }

int main()
{
	const int n = 600;
	std::vector<djb::vec3> i(n), o(n);
	std::vector<float> u1(n), u2(n);
	std::vector<int32_t> ids(n), local(n);
	const djb_scene_slot slots[5] = { { DJB_KIND_UTIA, 0 }, { DJB_KIND_SGD, 1 }, { DJB_SCENE_NONE, 0 }, { DJB_KIND_UTIA, 1 }, { DJB_KIND_SGD, 0 } };
	for (int k = 0; k < n; ++k) {
		const float ti = 1.5f * (float)((k * 7) % 64), pi_ = 7.5f * (float)((k * 5) % 48) + 0.37f * (float)(k % 11);      // up to 94.5 degrees: some below the horizon
		const float to = 1.5f * (float)((k * 11) % 64), po = 7.5f * (float)((k * 13) % 48) + 0.53f * (float)(k % 7);
		const float r = 0.017453292f;
		i[k] = djb::vec3(std::sin(ti * r) * std::cos(pi_ * r), std::sin(ti * r) * std::sin(pi_ * r), std::cos(ti * r));
		o[k] = djb::vec3(std::sin(to * r) * std::cos(po * r), std::sin(to * r) * std::sin(po * r), std::cos(to * r));
		u1[k] = (float)((k * 37) % 101) / 101.0f; u2[k] = (float)((k * 53) % 97) / 97.0f;
		const int32_t cycle[8] = { 0, 1, 2, 3, 4, -1, 5, 3 };            // 2: the slot without material; -1 and 5: outside the table
		ids[k] = cycle[k % 8];
		local[k] = ids[k] >= 0 && ids[k] < 5 && slots[ids[k]].kind != DJB_SCENE_NONE ? slots[ids[k]].local : -1;
	}
	std::vector<double> tab[2] = { std::vector<double>(3 * 288 * 288), std::vector<double>(3 * 288 * 288) };
	for (int m = 0; m < 2; ++m)
		for (size_t e = 0; e < tab[m].size(); ++e) tab[m][e] = 20.0 + 15.0 * std::sin(0.001 * (double)e * (m + 1)) + 5.0 * m;
	djb::utia ua(tab[0].data()), ub(tab[1].data());
	const djb::utia *um[2] = { &ua, &ub };
	djb::utia_set utia_set(2, um);
	if (utia_set.has_proxy_params()) return 3;                 // a new set has none
	const djb::microfacet::params up[2] = { djb::microfacet::params::isotropic(0.3f), djb::microfacet::params::elliptic(0.2f, 0.4f, 0.3f) };
	djb::sgd a("gold-metallic-paint"), b("blue-acrylic");
	const djb::sgd *members[2] = { &a, &b };
	djb::model_set sgd_set(2, members);
	sgd_set.fit_proxy(24, true);
	djb::scene sc(NULL, &utia_set, &sgd_set, NULL, 5, slots);
	djb::ggx lobe;
	std::vector<djb::vec3> w(n), si(n), fr(n);
	std::vector<float> pdf(n), lpdf(n);
	try {                                                      // the utia member has no parameters yet: refused, and the message names it
		sc.evalp_is_proxy(&lobe, (size_t)n, ids.data(), &u1[0], &u2[0], &o[0], &w[0], &si[0], &pdf[0]);
		return 4;
	} catch (const djb::exc &e) {
		if (!strstr(e.what(), "utia member")) return 5;
	}
	utia_set.set_proxy_params(up);                             // after the scene was built: the next call sees them
	if (!utia_set.has_proxy_params()) return 6;
	try {                                                      // a scene with a utia member needs the lobe
		sc.evalp_pdf_proxy(NULL, (size_t)n, ids.data(), &i[0], &o[0], &fr[0], &lpdf[0]);
		return 7;
	} catch (const djb::exc &) {
	}
	sc.evalp_is_proxy(&lobe, (size_t)n, ids.data(), &u1[0], &u2[0], &o[0], &w[0], &si[0], &pdf[0]);
	sc.evalp_pdf_proxy(&lobe, (size_t)n, ids.data(), &i[0], &o[0], &fr[0], &lpdf[0]);

	// the members' own answers: the model set on the local ids of its hits, the utia objects one by one
	std::vector<int32_t> sgd_ids(n);
	for (int k = 0; k < n; ++k) sgd_ids[k] = ids[k] >= 0 && ids[k] < 5 && slots[ids[k]].kind == DJB_KIND_SGD ? local[k] : -1;
	std::vector<djb::vec3> mw(n), mi(n), mfr(n);
	std::vector<float> mpdf(n), mlpdf(n);
	sgd_set.evalp_is_proxy((size_t)n, sgd_ids.data(), &u1[0], &u2[0], &o[0], &mw[0], &mi[0], &mpdf[0]);
	sgd_set.evalp_pdf_proxy((size_t)n, sgd_ids.data(), &i[0], &o[0], &mfr[0], &mlpdf[0]);
	int differ = 0, checked = 0, nonzero = 0;
	for (int k = 0; k < n; ++k) {
		djb::vec3 ww(0, 0, 0), wi(0, 0, 0), wfr(0, 0, 0);
		float wpdf = 0.0f, wlpdf = 0.0f;
		const bool in = ids[k] >= 0 && ids[k] < 5;
		if (in && slots[ids[k]].kind == DJB_KIND_UTIA) {
			const djb::utia &t = local[k] ? ub : ua;
			ww = t.evalp_is_proxy(lobe, u1[k], u2[k], o[k], &wi, &wpdf, NULL, &up[local[k]]);
			wfr = t.evalp_pdf_proxy(lobe, i[k], o[k], &wlpdf, NULL, &up[local[k]]);
		} else if (in && slots[ids[k]].kind == DJB_KIND_SGD) {
			ww = mw[k]; wi = mi[k]; wpdf = mpdf[k]; wfr = mfr[k]; wlpdf = mlpdf[k];
		}
		++checked;
		if (!same(w[k], ww) || !same(si[k], wi) || bits(pdf[k]) != bits(wpdf) || !same(fr[k], wfr) || bits(lpdf[k]) != bits(wlpdf)) ++differ;
		if (wpdf > 0.0f && ww.x != 0.0f) ++nonzero;
	}
	printf("%d hits checked, %d differ, %d non-zero\n", checked, differ, nonzero);
	return differ == 0 && nonzero > checked / 4 ? 0 : 1;
}
