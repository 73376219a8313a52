// model_set_proxy_facade.cpp -- the fitted proxies of djb::model_set (include/djb_hip.hpp): a set of two djb::sgd objects, fit_proxy(32),
// then proxy_table / evalp_is_proxy / evalp_pdf_proxy on a batch of hits (inactive ones included) held, bit for bit, against the
// single-material route through the C ABI: djb_brdf_create_tabular of each object, djb_tabular_get, djb_evalp_is_proxy_batch and
// djb_evalp_pdf_proxy_batch.  tests/test_model_set_proxy_host.py runs it on the CPU context (DJB_DEVICE=cpu).
// Prints "<n> values checked, <d> differ"; exit 1 if d != 0.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "dj_brdf.h"

static unsigned int bits(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
static int diff3(const djb::vec3 &a, const djb::vec3 &b) { return !(same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z)); }

int main()
{
	const int n = 600, RES = 32;
	std::vector<djb::vec3> i(n), o(n);
	std::vector<float> u1(n), u2(n);
	std::vector<int32_t> ids(n);
	for (int k = 0; k < n; ++k) {
		const float ti = 1.5f * (float)((k * 7) % 64), pi_ = 7.5f * (float)((k * 5) % 48) + 0.37f * (float)(k % 11);      // up to 94.5 degrees: some below the horizon
		const float to = 1.5f * (float)((k * 11) % 64), po = 7.5f * (float)((k * 13) % 48) + 0.53f * (float)(k % 7);
		const float r = 0.017453292f;
		i[k] = djb::vec3(std::sin(ti * r) * std::cos(pi_ * r), std::sin(ti * r) * std::sin(pi_ * r), std::cos(ti * r));
		o[k] = djb::vec3(std::sin(to * r) * std::cos(po * r), std::sin(to * r) * std::sin(po * r), std::cos(to * r));
		u1[k] = (float)((k * 37) % 101) / 100.0f; u2[k] = (float)((k * 53) % 97) / 96.0f;
		const int32_t cycle[5] = { 0, 1, -1, 1, 2 };          // 2 and -1: inactive
		ids[k] = cycle[k % 5];
	}
	djb::sgd a("gold-metallic-paint"), b("blue-acrylic");
	const djb::sgd *members[2] = { &a, &b };
	djb::model_set set(2, members);
	if (set.proxy_resolution() != 0) return 3;
	set.fit_proxy(RES, false);
	if (set.proxy_resolution() != RES || set.proxy_shadow()) return 4;
	djb_ctx *ctx = djb::hip::context::standard().get();
	int differ = 0, checked = 0, nonzero = 0;
	std::vector<djb::vec3> w(n), si(n), fr(n), ww(n), wi(n), wfr(n);
	std::vector<float> spdf(n), lpdf(n), wspdf(n), wlpdf(n);
	set.evalp_is_proxy((size_t)n, ids.data(), u1.data(), u2.data(), &o[0], &w[0], &si[0], spdf.data());
	set.evalp_pdf_proxy((size_t)n, ids.data(), &i[0], &o[0], &fr[0], lpdf.data());
	for (int m = 0; m < 2; ++m) {
		djb_brdf *tab = NULL;
		if (djb_brdf_create_tabular(ctx, members[m]->handle(), RES, 0, &tab) != DJB_OK) return 5;
		const int which[3] = { DJB_TAB_P22, DJB_TAB_SIGMA, DJB_TAB_QF };
		for (int t = 0; t < 3; ++t) {
			int cnt = 0;
			if (djb_tabular_get(tab, which[t], NULL, &cnt) != DJB_OK) return 6;
			std::vector<float> want((size_t)cnt), got = set.proxy_table(m, which[t]);
			if (cnt && djb_tabular_get(tab, which[t], want.data(), NULL) != DJB_OK) return 6;
			if ((int)got.size() != cnt) { ++differ; continue; }
			for (int e = 0; e < cnt; ++e) { ++checked; differ += !same(got[e], want[e]); }
		}
		djb_vec3_view vi = djb::hip::view(&i[0]), vo = djb::hip::view(&o[0]), vw = djb::hip::view(&ww[0]), vsi = djb::hip::view(&wi[0]), vfr = djb::hip::view(&wfr[0]);
		if (djb_evalp_is_proxy_batch(ctx, members[m]->handle(), tab, n, u1.data(), u2.data(), &vo, NULL, NULL, &vw, &vsi, wspdf.data(), DJB_MEM_HOST) != DJB_OK) return 7;
		if (djb_evalp_pdf_proxy_batch(ctx, members[m]->handle(), tab, n, &vi, &vo, NULL, NULL, &vfr, wlpdf.data(), DJB_MEM_HOST) != DJB_OK) return 8;
		for (int k = 0; k < n; ++k) {
			if (ids[k] != m) continue;
			checked += 5;
			differ += diff3(w[k], ww[k]) + diff3(si[k], wi[k]) + !same(spdf[k], wspdf[k]) + diff3(fr[k], wfr[k]) + !same(lpdf[k], wlpdf[k]);
			if (wspdf[k] > 0.0f && wlpdf[k] > 0.0f) ++nonzero;
		}
		djb_brdf_destroy(tab);
	}
	for (int k = 0; k < n; ++k)
		if (ids[k] != 0 && ids[k] != 1) {
			checked += 5;
			differ += (bits(w[k].x) | bits(w[k].y) | bits(w[k].z) | bits(si[k].x) | bits(si[k].y) | bits(si[k].z) | bits(spdf[k])) != 0;
			differ += (bits(fr[k].x) | bits(fr[k].y) | bits(fr[k].z) | bits(lpdf[k])) != 0;
		}
	printf("%d values checked, %d differ, %d hits with both pdfs positive\n", checked, differ, nonzero);
	return differ == 0 && nonzero > n / 8 ? 0 : 1;
}
