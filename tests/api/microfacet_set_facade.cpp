// microfacet_set_facade.cpp -- djb::microfacet_set of the djb:: facade (include/djb_hip.hpp): a set built from three djb::ggx objects with
// their own params, and a set built from two plain beckmann descriptions; eval / evalp / pdf / eval_pdf / sample / evalp_is of a batch of
// hits (inactive ones included) held, bit for bit, against the single-material objects' own one-pair calls with the same params.
// tests/test_microfacet_set_host.py runs it on the CPU context (DJB_DEVICE=cpu).  Prints "<n> hits checked, <d> differ"; exit 1 if d != 0.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "dj_brdf.h"

static unsigned int bits(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
static bool same(const djb::vec3 &a, const djb::vec3 &b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }

int main()
{
	const int n = 600;
	std::vector<djb::vec3> i(n), o(n), fr(n), fr2(n), w(n), si(n), si2(n);
	std::vector<float> pdf(n), pdf2(n), ipdf(n), u1(n), u2(n);
	std::vector<int32_t> ids(n);
	for (int k = 0; k < n; ++k) {
		const float ti = 1.5f * (float)((k * 7) % 64), pi_ = 7.5f * (float)((k * 5) % 48) + 0.37f * (float)(k % 11);      // up to 94.5 degrees: some below the horizon
		const float to = 1.5f * (float)((k * 11) % 64), po = 7.5f * (float)((k * 13) % 48) + 0.53f * (float)(k % 7);
		const float r = 0.017453292f;
		i[k] = djb::vec3(std::sin(ti * r) * std::cos(pi_ * r), std::sin(ti * r) * std::sin(pi_ * r), std::cos(ti * r));
		o[k] = djb::vec3(std::sin(to * r) * std::cos(po * r), std::sin(to * r) * std::sin(po * r), std::cos(to * r));
		u1[k] = (float)((k * 37) % 101) / 100.0f; u2[k] = (float)((k * 53) % 103) / 102.0f;
		const int32_t cycle[7] = { 0, 1, -1, 2, 1, 3, 0 };    // 3 and -1: inactive
		ids[k] = cycle[k % 7];
	}
	int differ = 0, checked = 0, nonzero = 0;
	// ---- from objects: three ggx lobes, three Fresnel kinds, shadowing on and off
	const djb::microfacet::params p[3] = { djb::microfacet::params::isotropic(0.3f), djb::microfacet::params::elliptic(0.2f, 0.5f, 0.7f),
	                                       djb::microfacet::params::pdfparams(0.4f, 0.25f, 0.3f, 0.1f, -0.05f) };
	djb::ggx a(djb::fresnel::ideal(), true), b(djb::fresnel::schlick(djb::vec3(1.0f, 0.71f, 0.29f)), false),
	         c(djb::fresnel::unpolarized(djb::vec3(1.5f, 1.8f, 2.4f)), true);
	const djb::microfacet *single[3] = { &a, &b, &c };
	djb::microfacet_set *set;
	{
		djb::ggx a2(djb::fresnel::ideal(), true), b2(djb::fresnel::schlick(djb::vec3(1.0f, 0.71f, 0.29f)), false),
		         c2(djb::fresnel::unpolarized(djb::vec3(1.5f, 1.8f, 2.4f)), true);
		const djb::microfacet *members[3] = { &a2, &b2, &c2 };
		set = new djb::microfacet_set(3, members, p);         // the members go out of scope: the set holds copies
	}
	if (set->size() != 3 || set->kind() != DJB_KIND_GGX) return 3;
	djb::microfacet_set moved(std::move(*set));               // move-only
	delete set;
	if (moved.size() != 3) return 4;
	for (int cosine = 0; cosine < 2; ++cosine) {
		if (cosine) moved.evalp((size_t)n, ids.data(), &i[0], &o[0], &fr[0]);
		else moved.eval((size_t)n, ids.data(), &i[0], &o[0], &fr[0]);
		moved.eval_pdf((size_t)n, ids.data(), &i[0], &o[0], &fr2[0], &pdf2[0], cosine != 0);
		moved.pdf((size_t)n, ids.data(), &i[0], &o[0], &pdf[0]);
		for (int k = 0; k < n; ++k) {
			djb::vec3 want(0, 0, 0); float want_pdf = 0.0f;
			if (ids[k] >= 0 && ids[k] < 3) {
				const djb::microfacet &m = *single[ids[k]];
				want = cosine ? m.evalp(i[k], o[k], &p[ids[k]]) : m.eval(i[k], o[k], &p[ids[k]]);
				want_pdf = m.pdf(i[k], o[k], &p[ids[k]]);
			}
			++checked;
			if (!same(fr[k], want) || !same(fr2[k], want) || !same(pdf[k], want_pdf) || !same(pdf2[k], want_pdf)) ++differ;
			if (want.x != 0.0f && want.x == want.x) ++nonzero;
		}
	}
	moved.evalp_is((size_t)n, ids.data(), &u1[0], &u2[0], &o[0], &w[0], &si[0], &ipdf[0]);
	moved.sample((size_t)n, ids.data(), &u1[0], &u2[0], &o[0], &si2[0]);
	for (int k = 0; k < n; ++k) {
		djb::vec3 want_w(0, 0, 0), want_i(0, 0, 0), want_s(0, 0, 0); float want_pdf = 0.0f;
		if (ids[k] >= 0 && ids[k] < 3) {
			const djb::microfacet &m = *single[ids[k]];
			want_w = m.evalp_is(u1[k], u2[k], o[k], &want_i, &want_pdf, &p[ids[k]]);
			want_s = m.sample(u1[k], u2[k], o[k], &p[ids[k]]);
		}
		++checked;
		if (!same(w[k], want_w) || !same(si[k], want_i) || !same(ipdf[k], want_pdf) || !same(si2[k], want_s)) ++differ;
	}
	// ---- from plain descriptions: two beckmann materials; then set_params
	djb_microfacet_material mats[2];
	memset(mats, 0, sizeof mats);
	mats[0].fresnel.kind = DJB_FRESNEL_SCHLICK; mats[0].fresnel.a[0] = 0.9f; mats[0].fresnel.a[1] = 0.5f; mats[0].fresnel.a[2] = 0.1f;
	mats[0].shadow = 1; mats[0].params.kind = DJB_PARAMS_ELLIPTIC; mats[0].params.v[0] = 0.3f; mats[0].params.v[1] = 0.3f;
	mats[1].fresnel.kind = DJB_FRESNEL_IDEAL; mats[1].shadow = 0;                                   // params: standard
	djb::microfacet_set bk(DJB_KIND_BECKMANN, 2, mats);
	if (bk.size() != 2 || bk.kind() != DJB_KIND_BECKMANN) return 5;
	djb::beckmann b0(djb::fresnel::schlick(djb::vec3(0.9f, 0.5f, 0.1f)), true), b1(djb::fresnel::ideal(), false);
	const djb::microfacet *bsingle[2] = { &b0, &b1 };
	djb::microfacet::params bp[2] = { djb::microfacet::params::isotropic(0.3f), djb::microfacet::params::standard() };
	for (int round = 0; round < 2; ++round) {
		bk.evalp((size_t)n, ids.data(), &i[0], &o[0], &fr[0]);
		for (int k = 0; k < n; ++k) {
			djb::vec3 want(0, 0, 0);
			if (ids[k] == 0 || ids[k] == 1) want = bsingle[ids[k]]->evalp(i[k], o[k], &bp[ids[k]]);
			++checked;
			if (!same(fr[k], want)) ++differ;
			if (want.x != 0.0f && want.x == want.x) ++nonzero;
		}
		bp[0] = djb::microfacet::params::pdfparams(0.3f, 0.2f, 0.4f, 0.5f, -0.3f); bp[1] = djb::microfacet::params::elliptic(0.2f, 0.5f, 0.7f);
		bk.set_params(bp);                                    // seen by the next call
	}
	printf("%d hits checked, %d differ, %d non-zero\n", checked, differ, nonzero);
	return differ == 0 && nonzero > checked / 8 ? 0 : 1;
}
